"""Tensor-level wrappers over the C ABI (one function per entry point).

Every wrapper takes contiguous fp32 CUDA(HIP) tensors, allocates outputs with torch
(plumbing only: the caching allocator and the current stream), and enqueues the HIP
kernel on ``torch.cuda.current_stream()``.  There is no CPU or ATen fallback: a CPU
tensor raises.
"""
import ctypes
import operator

import numpy as np
import torch

from . import _lib
from . import layout
from ._lib import ACT_NONE, ACT_TANH, PAD_REFLECT, PAD_ZERO, SeganSrc, check


import os as _os

_D = _lib.DEFINES       # the integer macros of include/segan_hip.h
PREC_FP32, PREC_BF16, PREC_BF16X3 = _D['SEGAN_PREC_FP32'], _D['SEGAN_PREC_BF16'], _D['SEGAN_PREC_BF16X3']
_PREC_NAMES = {'fp32': PREC_FP32, 'bf16': PREC_BF16, 'bf16x3': PREC_BF16X3}
_precision = _PREC_NAMES[_os.environ.get('SEGAN_PRECISION', 'fp32')]
_EUNSUPPORTED = -3


_deterministic = _os.environ.get('SEGAN_DETERMINISTIC', '0') == '1'


def set_deterministic(on):
    """Bit-reproducible mode.  The forward / data-gradient contractions always are reproducible
    (their stream-K tail is reduced in a fixed order); this switch makes the weight gradients and
    the dense-head GEMMs reduce their contraction splits in a fixed order too (slabs + a second
    kernel) instead of with fp32 atomics.  Measured cost: 11 % of the step in round 2, 0.6 - 2.2 % in
    rounds 3 - 5, 0.4 % at the end of round 6 (one box; the ordered reductions now issue their loads
    before their stores) — the first reading below the 1 % at which it would become the default, so
    it stays opt-in until that holds across boxes: ``set_deterministic(True)`` /
    SEGAN_DETERMINISTIC=1 / train.py --deterministic.  (The
    bf16 / bf16x3 weight gradients always add their splits with atomics.)"""
    global _deterministic
    _deterministic = bool(on)


def get_deterministic():
    return _deterministic


_ACC_NAMES = ('plain', 'blocked')
_accumulation = _os.environ.get('SEGAN_ACCUMULATION', 'plain')
if _accumulation not in _ACC_NAMES:
    raise ValueError('SEGAN_ACCUMULATION must be one of {}'.format(_ACC_NAMES))
PREC_FP32_BLOCKED = _D['SEGAN_PREC_FP32_BLOCKED']


def set_accumulation(mode):
    """How the fp32 forward / data-gradient contractions accumulate: 'plain' (one MFMA
    accumulator over the whole contraction: the default and the benchmarked configuration) or
    'blocked' (SEGAN_PREC_FP32_BLOCKED: 256-term blocks summed in a second register set).
    Blocked accumulation brings the forward error of the deep layers against fp64 from
    1.5-2.2e-6 down to 3e-7 — below torch's own CPU fp32 result.  It costs one of the three
    resident waves per SIMD (~3 % of the contraction rate, 1.5-2.2 % of the step), so it is
    opt-in: ``set_accumulation('blocked')`` / SEGAN_ACCUMULATION=blocked.  What it does NOT
    buy is a reliably smaller batch-300 gradient distance to the oracle: that figure is set by
    which individual PReLU gates flip, not by the size of the roundoff.
    The weight gradients stay plain (their contractions are split across workgroups already;
    blocking them was measured: no change in any parity figure for 4.4 % of the step).  No
    effect on the bf16 modes."""
    global _accumulation
    if mode not in _ACC_NAMES:
        raise ValueError('accumulation must be one of {}'.format(_ACC_NAMES))
    _accumulation = mode


def get_accumulation():
    return _accumulation


def _fp32():
    return PREC_FP32_BLOCKED if _accumulation == 'blocked' else PREC_FP32


def set_precision(mode):
    """Precision of ALL contractions (conv / deconv forward, data gradients and weight
    gradients): 'fp32' (exact fp32 MFMA, the default and the benchmarked configuration), 'bf16'
    (bf16 operands, fp32 accumulate: BASELINE config 5) or 'bf16x3' (exact 3-way bf16 split of
    every fp32 operand, six partial products: fp32-class accuracy on the bf16 matrix cores).
    A geometry the bf16 kernels do not cover falls back to fp32 per call.  The dense head,
    BatchNorm, activations, losses and optimizers always run in fp32."""
    global _precision
    if mode not in _PREC_NAMES:
        raise ValueError('precision must be one of {}'.format(sorted(_PREC_NAMES)))
    _precision = _PREC_NAMES[mode]


def get_precision():
    return [k for k, v in _PREC_NAMES.items() if v == _precision][0]


def _stream():
    # the raw handle of torch's current stream on the current device: two C calls (torch.cuda.
    # current_stream() builds a python Stream object per call: 3 us, twice per library call)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _ptr(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _chk(t, name, ndim=None, dtype=torch.float32, contiguous=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError('{} must be a tensor, got {}'.format(name, type(t)))
    if not t.is_cuda:
        raise RuntimeError(
            '{} is on {}: segan_pytorch_amd runs only on an MI355X (HIP) device; '
            'there is no CPU path'.format(name, t.device))
    if t.dtype != dtype:
        raise TypeError('{} must be {}, got {}'.format(name, str(dtype)[len('torch.'):], t.dtype))
    if contiguous and not t.is_contiguous():
        raise ValueError('{} must be contiguous'.format(name))
    if ndim is not None and t.dim() != ndim:
        raise ValueError('{} must have {} dims, got {}'.format(name, ndim, tuple(t.shape)))
    return t


def _chk_pair(what, ref, deg):
    """ref and deg are fp32 CUDA [rows, T] of one shape; returns (rows, T)."""
    _chk(ref, 'ref', 2)
    _chk(deg, 'deg', 2)
    if ref.shape != deg.shape:
        raise ValueError('{}: shapes differ {} vs {}'.format(what, tuple(ref.shape), tuple(deg.shape)))
    return ref.shape


class Src(object):
    """A logical [B, C0+C1, L] activation with an on-load transform (``segan_src``).

    ``t0``/``t1``: the channel segments; ``scale``/``shift``/``slope``: optional
    per-channel vectors over the concatenated channel axis.
    """

    def __init__(self, t0, t1=None, scale=None, shift=None, slope=None):
        _chk(t0, 'src.t0', 3)
        self.t0, self.t1 = t0, t1
        self.C0 = t0.shape[1]
        self.C1 = 0
        if t1 is not None:
            _chk(t1, 'src.t1', 3)
            if t1.shape[0] != t0.shape[0] or t1.shape[2] != t0.shape[2]:
                raise ValueError('src segments disagree: {} vs {}'.format(
                    tuple(t0.shape), tuple(t1.shape)))
            self.C1 = t1.shape[1]
        self.C = self.C0 + self.C1
        for name, v in (('scale', scale), ('shift', shift), ('slope', slope)):
            if v is not None:
                _chk(v, 'src.' + name)
                if v.numel() != self.C:
                    raise ValueError('src.{} has {} entries for {} channels'.format(
                        name, v.numel(), self.C))
        self.scale, self.shift, self.slope = scale, shift, slope
        self.B, self.L = t0.shape[0], t0.shape[2]

    def c_struct(self):
        s = SeganSrc()
        s.p0 = self.t0.data_ptr()
        s.p1 = self.t1.data_ptr() if self.t1 is not None else None
        s.C0, s.C1 = self.C0, self.C1
        s.scale = self.scale.data_ptr() if self.scale is not None else None
        s.shift = self.shift.data_ptr() if self.shift is not None else None
        s.slope = self.slope.data_ptr() if self.slope is not None else None
        return s


# stream-K scratch of the fp32 contractions (include/segan_hip.h): one buffer per device and
# stream (launches on different streams must not share it), allocated on first use
_corr_scratch = {}


def _scratch():
    """(pointer, bytes) of this device+stream's stream-K scratch."""
    dev = torch._C._cuda_getDevice()
    key = (dev, torch._C._cuda_getCurrentRawStream(dev))
    buf = _corr_scratch.get(key)
    if buf is None:
        nbytes = _lib.load().segan_corr_scratch_bytes()
        buf = torch.empty(nbytes, device=torch.device('cuda', dev), dtype=torch.uint8)
        _corr_scratch[key] = buf
    return ctypes.c_void_p(buf.data_ptr()), buf.numel()


def last_corr_launch():
    """Diagnostics: dict describing this thread's last fp32 conv / deconv forward or data
    gradient launch (segan_debug_last_corr)."""
    arr = (ctypes.c_int * 6)()
    _lib.load().segan_debug_last_corr(arr)
    k = ('kernel', 'workgroups', 'tiles', 'tiles_whole', 'streamk_units', 'xf_mode')
    d = dict(zip(k, list(arr)))
    d['streamk'] = d['streamk_units'] > 0
    return d


def last_wgrad_launch():
    """Diagnostics: how this thread's last fp32 weight gradient was launched."""
    arr = (ctypes.c_int * 6)()
    _lib.load().segan_debug_last_wgrad(arr)
    return dict(zip(('kernel', 'tiles', 'splits', 'chunks_per_split', 'resident_per_cu', 'hi_loads'),
                    list(arr)))


_call_scratch = {}


def _stream_scratch(nbytes, device):
    """A per-call scratch buffer of at least `nbytes` on this device + stream: ONE grow-only
    buffer per (device, stream), re-used by every call — the calls of a stream execute in order
    and none keeps its scratch past its last kernel (round-3 advice: a fresh torch.empty of
    134+ MB per bf16 contraction call went through the caching allocator thousands of times per
    step)."""
    dev = torch.device(device).index
    if dev is None:
        dev = torch._C._cuda_getDevice()
    key = (dev, torch._C._cuda_getCurrentRawStream(dev))
    buf = _call_scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _call_scratch.pop(key, None)          # release before growing
        buf = torch.empty(int(nbytes), device=torch.device('cuda', dev), dtype=torch.uint8)
        _call_scratch[key] = buf
    return buf


def set_reserved_slots(n):
    """Workgroup slots the launch planners of the contraction kernels leave free for other kernels
    (segan_set_reserved_slots; default 0 or $SEGAN_RESERVED_SLOTS): RCCL's channels during a
    data-parallel step.  Returns the previous value."""
    return int(_lib.load().segan_set_reserved_slots(int(n)))


def release_scratch(device=None):
    """Hand the per-stream scratch buffers (the stream-K slabs of the fp32 contractions, 128 MiB
    per device + stream, and the grow-only call scratch of the bf16 / weight-gradient calls, 134+ MB
    per stream) back to the caching allocator — all of them, or those of one device.

    The buffers are keyed by the RAW stream handle, so an entry outlives a destroyed torch stream;
    nothing else ever frees them.  Call it where streams come and go (a server that creates a
    stream per request) or before handing the device to something else; the next contraction call
    re-allocates what it needs.  Safe at any point between calls: the kernels that used a buffer
    were enqueued on its stream, and the caching allocator re-uses the block in stream order
    (the buffers were allocated while their stream was current).

    The invariant the sharing rests on, stated here because nothing else enforces it: a library
    call hands out AT MOST ONE region of a stream's call scratch (`_stream_scratch`), and no call
    keeps it past its last kernel.  A bf16 call that the library declines (SEGAN_EUNSUPPORTED) and
    that is retried in fp32 satisfies it because the fp32 forms use `_scratch()` — the separate
    stream-K buffer — only."""
    dev = None if device is None else torch.device(device).index
    for d in (_corr_scratch, _call_scratch):
        for key in [k for k in d if dev is None or k[0] == dev]:
            del d[key]


def scratch_bytes():
    """Bytes currently held by the per-stream scratch buffers (diagnostics / tests)."""
    return sum(b.numel() for d in (_corr_scratch, _call_scratch) for b in d.values())


def _bf_scratch(op, B, N, M, L, K, S, pad, device):
    """(buffer, pointer, bytes) of the packed-activation scratch of a bf16 / bf16x3 contraction
    call (segan_bf16_scratch_bytes), from the stream's call scratch."""
    planes = 3 if _precision == PREC_BF16X3 else 1
    nbytes = _lib.load().segan_bf16_scratch_bytes(op, B, N, M, L, K, S, pad, planes)
    if nbytes == 0:
        return None, None, 0
    buf = _stream_scratch(nbytes, device)
    return buf, ctypes.c_void_p(buf.data_ptr()), nbytes


def conv_pad(K, S):
    return layout.conv_pad(K, S)


def deconv_pad(K, S):
    return layout.deconv_pad(K, S)


# ---------------------------------------------------------------------------------
# weight packing
# ---------------------------------------------------------------------------------
_weights_epoch = 0


def bump_weights_epoch(params=None):
    """Invalidate packed weights after the weights were modified through raw pointers (the
    fused optimizers, DP broadcast), which torch's version counter cannot see.  With
    `params` only those tensors' packs are invalidated (an optimizer step must not force
    the OTHER network to re-pack); without, every WeightPack is."""
    global _weights_epoch
    if params is None:
        _weights_epoch += 1
        return
    for p in params:
        p._segan_epoch = getattr(p, '_segan_epoch', 0) + 1


class WeightPack(object):
    """Polyphase-packed copies of ONE weight tensor [m, n, K] (see layout.py), owned by
    the module that owns the weight and refreshed when the weight changes."""

    def __init__(self):
        self._buf = {}
        self._key = {}

    def _get(self, w, S, pad_t, want):
        _chk(w, 'weight', 3)
        key = (w.data_ptr(), w._version, _weights_epoch, getattr(w, '_segan_epoch', 0),
               tuple(w.shape), S, pad_t)
        if self._key.get(want) == key:
            return self._buf[want]
        lib = _lib.load()
        M, N, K = w.shape
        nbytes = (lib.segan_packed_f_bytes if want == 'f' else lib.segan_packed_t_bytes)(M, N, S)
        if nbytes == 0:
            raise ValueError('unsupported stride {} (must be 1, 2 or 4)'.format(S))
        buf = self._buf.get(want)
        if buf is None or buf.numel() * 4 != nbytes or buf.device != w.device:
            buf = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
        check(lib.segan_pack_weights(_ptr(w), _ptr(buf) if want == 'f' else None,
                                     _ptr(buf) if want == 't' else None, M, N, K, S, pad_t,
                                     _stream()), 'pack_weights')
        self._buf[want] = buf
        self._key[want] = key
        return buf

    def f(self, w, S):
        return self._get(w, S, 0, 'f')

    def g(self, w, S):
        """"G" packing wg[m][n*32 + r*8 + u] = w[m][n][4u + r] of the short-row data gradient
        (segan_pack_weights_g)."""
        _chk(w, 'weight', 3)
        key = (w.data_ptr(), w._version, _weights_epoch, getattr(w, '_segan_epoch', 0),
               tuple(w.shape), S)
        if self._key.get('g') == key:
            return self._buf['g']
        lib = _lib.load()
        M, N, K = w.shape
        nbytes = lib.segan_packed_g_bytes(M, N, S)
        if nbytes == 0:
            raise ValueError('G packing: stride {} not supported'.format(S))
        buf = self._buf.get('g')
        if buf is None or buf.numel() * 4 != nbytes or buf.device != w.device:
            buf = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
        check(lib.segan_pack_weights_g(_ptr(w), _ptr(buf), M, N, K, S, _stream()), 'pack_weights_g')
        self._buf['g'] = buf
        self._key['g'] = key
        return buf

    def t(self, w, S, pad_t):
        return self._get(w, S, pad_t, 't')

    def bf(self, w, S, pad_t, tform, planes):
        """bf16-plane packing (segan_pack_weights_bf) for the bf16 / bf16x3 kernels."""
        _chk(w, 'weight', 3)
        want = ('bf', tform, planes)
        key = (w.data_ptr(), w._version, _weights_epoch, getattr(w, '_segan_epoch', 0),
               tuple(w.shape), S, pad_t)
        if self._key.get(want) == key:
            return self._buf[want]
        lib = _lib.load()
        M, N, K = w.shape
        nbytes = lib.segan_packed_bf_bytes(M, N, S, tform, planes)
        if nbytes == 0:
            raise ValueError('unsupported geometry for bf16 packing')
        buf = self._buf.get(want)
        if buf is None or buf.numel() * 2 != nbytes or buf.device != w.device:
            buf = torch.empty(nbytes // 2, device=w.device, dtype=torch.bfloat16)
        check(lib.segan_pack_weights_bf(_ptr(w), _ptr(buf), M, N, K, S, tform, pad_t, planes,
                                        _stream()), 'pack_weights_bf')
        self._buf[want] = buf
        self._key[want] = key
        return buf


# ---------------------------------------------------------------------------------
# contractions
# ---------------------------------------------------------------------------------
def conv1d_fwd(src, w, bias, S, roll=0, pad_mode=PAD_REFLECT, padL=None, pack=None):
    """Pre-activation of GConv1DBlock: conv(reflect_pad(roll(src)), w) + bias."""
    M, N, K = w.shape
    if src.C != N:
        raise ValueError('conv1d_fwd: input has {} channels, weight expects {}'.format(src.C, N))
    B, L = src.B, src.L
    if L % S != 0:
        raise ValueError('conv1d_fwd: length {} not divisible by stride {}'.format(L, S))
    if padL is None:
        padL = conv_pad(K, S)[0]
    out = torch.empty((B, M, L // S), device=w.device, dtype=torch.float32)
    cs = src.c_struct()
    pack = pack or WeightPack()
    lib = _lib.load()
    if _precision and pad_mode == PAD_REFLECT:
        keep, sp, sn = _bf_scratch(0, B, N, M, L, K, S, padL, w.device)
        rc = lib.segan_conv1d_fwd(ctypes.byref(cs), _ptr(pack.bf(w, S, 0, 0, _precision)),
                                  _ptr(bias), _ptr(out), B, N, M, L, K, S, padL, pad_mode, roll,
                                  _precision, sp, sn, _stream())
        if rc != _EUNSUPPORTED:
            check(rc, 'conv1d_fwd')
            return out
    check(lib.segan_conv1d_fwd(ctypes.byref(cs), _ptr(pack.f(w, S)), _ptr(bias), _ptr(out), B, N,
                               M, L, K, S, padL, pad_mode, roll, _fp32(), *_scratch(), _stream()),
          'conv1d_fwd')
    return out


def conv1d_dgrad(da, w, L, S, roll=0, padL=None, pack=None):
    """Gradient of conv1d_fwd w.r.t. its (un-rolled, un-padded) input: [B, N, L]."""
    _chk(da, 'da', 3)
    M, N, K = w.shape
    B = da.shape[0]
    if da.shape[1] != M or da.shape[2] * S != L:
        raise ValueError('conv1d_dgrad: da {} inconsistent with weight {} / L {}'.format(
            tuple(da.shape), tuple(w.shape), L))
    if padL is None:
        padL = conv_pad(K, S)[0]
    small = N <= 2          # first layer: direct VALU kernel on the unpacked weight
    _chk(w, 'weight', 3)
    pack = pack or WeightPack()
    if not small and not _precision and short_rows_ok(N, M, L, S):
        # deep layers (at most 64 positions per row after the stride): GEMM + col2im form, no
        # zero-halo columns, fold and roll in the epilogue
        return conv1d_dgrad_short(da, w, L, S, roll=roll, padL=padL, pack=pack)
    dx = torch.empty((B, N, L), device=da.device, dtype=torch.float32)
    halo = torch.empty((B * N * max(K - 1, 1),), device=da.device, dtype=torch.float32)
    lib = _lib.load()
    if small:
        check(lib.segan_conv1d_dgrad(_ptr(da), None, _ptr(w.detach()), _ptr(dx), _ptr(halo), B, N,
                                     M, L, K, S, padL, roll, PREC_FP32, None, 0, _stream()),
              'conv1d_dgrad')
        return dx
    if _precision:
        keep, sp, sn = _bf_scratch(1, B, N, M, L, K, S, padL, da.device)
        rc = lib.segan_conv1d_dgrad(_ptr(da), _ptr(pack.bf(w, S, 0, 1, _precision)), None, _ptr(dx),
                                    _ptr(halo), B, N, M, L, K, S, padL, roll, _precision, sp, sn,
                                    _stream())
        if rc != _EUNSUPPORTED:
            check(rc, 'conv1d_dgrad')
            return dx
    if short_rows_ok(N, M, L, S):        # a bf16 mode whose kernel does not cover this geometry
        return conv1d_dgrad_short(da, w, L, S, roll=roll, padL=padL, pack=pack)
    check(lib.segan_conv1d_dgrad(_ptr(da), _ptr(pack.t(w, S, 0)), None, _ptr(dx), _ptr(halo), B, N,
                                 M, L, K, S, padL, roll, _fp32(), *_scratch(), _stream()),
          'conv1d_dgrad')
    return dx


def conv1d_dgrad_short(da, w, L, S, roll=0, padL=None, pack=None):
    """conv1d_dgrad through segan_conv1d_dgrad_short (L/S in {4, 8, 16, 32, 64}, N % 4 == 0,
    M % 16 == 0); raises for other geometries."""
    _chk(da, 'da', 3)
    _chk(w, 'weight', 3)
    M, N, K = w.shape
    B = da.shape[0]
    if padL is None:
        padL = conv_pad(K, S)[0]
    dx = torch.empty((B, N, L), device=da.device, dtype=torch.float32)
    pack = pack or WeightPack()
    check(_lib.load().segan_conv1d_dgrad_short(_ptr(da), _ptr(pack.g(w, S)), _ptr(dx), B, N,
                                               M, L, K, S, padL, roll, _stream()),
          'conv1d_dgrad_short')
    return dx


_SHORT_LS = (4, 8, 16, 32, 64)


def short_rows_ok(N, M, L, S):
    """Does the fp32 conv data gradient of this geometry run the short-row kernel
    (segan_conv1d_dgrad_short)?"""
    return S in (2, 4) and L % S == 0 and (L // S) in _SHORT_LS and N % 4 == 0 and M % 16 == 0


def wgrad(lo, hi, dw, K, S, padL, pad_mode, roll=0):
    """dw[m,n,k] += sum lo[b,m,t] * pad(roll(hi))[b,n,S*t+k]  (accumulates into dw)."""
    _chk(dw, 'dw', 3)
    M, N = lo.C, hi.C
    if tuple(dw.shape) != (M, N, K):
        raise ValueError('wgrad: dw {} != ({}, {}, {})'.format(tuple(dw.shape), M, N, K))
    if lo.B != hi.B or lo.L * S != hi.L:
        raise ValueError('wgrad: lo [{}x{}] / hi [{}x{}] inconsistent for stride {}'.format(
            lo.B, lo.L, hi.B, hi.L, S))
    cl, ch = lo.c_struct(), hi.c_struct()
    lib = _lib.load()
    if _precision != PREC_FP32:
        nbytes = lib.segan_wgrad_scratch_bytes(lo.B, M, N, lo.L, S, _precision, 0)
        scratch = _stream_scratch(nbytes, dw.device)
        rc = lib.segan_wgrad(ctypes.byref(cl), ctypes.byref(ch), _ptr(dw), lo.B, M, N, lo.L, K, S,
                             padL, pad_mode, roll, _precision, 0,
                             ctypes.c_void_p(scratch.data_ptr()) if scratch is not None else None,
                             nbytes if scratch is not None else 0, _stream())
        if rc != -3:
            check(rc, 'wgrad')
            return
    flags = 1 if _deterministic else 0
    lo_plain = lo.t1 is None and lo.scale is None and lo.shift is None and lo.slope is None
    scratch, nbytes = None, 0
    if flags or not lo_plain:
        nbytes = lib.segan_wgrad_scratch_bytes(lo.B, M, N, lo.L, S, PREC_FP32, flags)
        scratch = _stream_scratch(nbytes, dw.device)
    check(lib.segan_wgrad(ctypes.byref(cl), ctypes.byref(ch), _ptr(dw), lo.B, M, N, lo.L, K, S, padL,
                          pad_mode, roll, PREC_FP32, flags,
                          ctypes.c_void_p(scratch.data_ptr()) if scratch is not None else None, nbytes,
                          _stream()), 'wgrad')


def deconv1d_fwd(src, w, bias, S, act=ACT_NONE, pack=None):
    """GDeconv1DBlock pre-activation (or tanh output): [B, N, S*Ls]."""
    M, N, K = w.shape
    if src.C != M:
        raise ValueError('deconv1d_fwd: input has {} channels, weight expects {}'.format(src.C, M))
    pad = deconv_pad(K, S)
    B, Ls = src.B, src.L
    y = torch.empty((B, N, S * Ls), device=w.device, dtype=torch.float32)
    cs = src.c_struct()
    small = N <= 2          # last generator layer (Cout = 1): direct VALU kernel
    _chk(w, 'weight', 3)
    pack = pack or WeightPack()
    lib = _lib.load()
    if small:
        check(lib.segan_deconv1d_fwd(ctypes.byref(cs), None, _ptr(w.detach()), _ptr(bias), _ptr(y),
                                     B, M, N, Ls, K, S, pad, act, PREC_FP32, None, 0, _stream()),
              'deconv1d_fwd')
        return y
    if _precision and act == ACT_NONE:
        keep, sp, sn = _bf_scratch(2, B, N, M, S * Ls, K, S, pad, w.device)
        rc = lib.segan_deconv1d_fwd(ctypes.byref(cs), _ptr(pack.bf(w, S, pad, 1, _precision)), None,
                                    _ptr(bias), _ptr(y), B, M, N, Ls, K, S, pad, act, _precision,
                                    sp, sn, _stream())
        if rc != _EUNSUPPORTED:
            check(rc, 'deconv1d_fwd')
            return y
    check(lib.segan_deconv1d_fwd(ctypes.byref(cs), _ptr(pack.t(w, S, pad)), None, _ptr(bias),
                                 _ptr(y), B, M, N, Ls, K, S, pad, act, _fp32(), *_scratch(),
                                 _stream()), 'deconv1d_fwd')
    return y


def deconv1d_dgrad(dy, w, S, M0=0, need0=True, need1=True, pack=None):
    """Gradient w.r.t. the deconv input, split at channel M0 into (dx0, dx1)."""
    _chk(dy, 'dy', 3)
    M, N, K = w.shape
    B = dy.shape[0]
    if dy.shape[1] != N or dy.shape[2] % S != 0:
        raise ValueError('deconv1d_dgrad: dy {} inconsistent with weight {}'.format(
            tuple(dy.shape), tuple(w.shape)))
    Ls = dy.shape[2] // S
    pad = deconv_pad(K, S)
    dx0 = dx1 = None
    if M0 > 0 and need0:
        dx0 = torch.empty((B, M0, Ls), device=dy.device, dtype=torch.float32)
    if M - M0 > 0 and need1:
        dx1 = torch.empty((B, M - M0, Ls), device=dy.device, dtype=torch.float32)
    if dx0 is None and dx1 is None:
        return None, None
    pack = pack or WeightPack()
    lib = _lib.load()
    if _precision:
        keep, sp, sn = _bf_scratch(3, B, N, M, S * Ls, K, S, pad, dy.device)
        rc = lib.segan_deconv1d_dgrad(_ptr(dy), _ptr(pack.bf(w, S, 0, 0, _precision)), _ptr(dx0),
                                      _ptr(dx1), B, M, M0, N, Ls, K, S, pad, _precision, sp, sn,
                                      _stream())
        if rc != _EUNSUPPORTED:
            check(rc, 'deconv1d_dgrad')
            return dx0, dx1
    check(lib.segan_deconv1d_dgrad(_ptr(dy), _ptr(pack.f(w, S)), _ptr(dx0), _ptr(dx1), B, M, M0, N,
                                   Ls, K, S, pad, _fp32(), *_scratch(), _stream()), 'deconv1d_dgrad')
    return dx0, dx1


# ---------------------------------------------------------------------------------
# per-channel kernels
# ---------------------------------------------------------------------------------
def _ws(B, C, L, per_split, extra, device):
    ns = _lib.load().segan_bn_nsplit(B, C, L)
    return torch.empty((per_split * ns * C + extra * C,), device=device, dtype=torch.float32)


def bn_stats(x, gamma, beta, eps, momentum, running_mean, running_var):
    """Training-mode BatchNorm1d statistics; returns (mean, rstd, scale, shift)."""
    _chk(x, 'x', 3)
    B, C, L = x.shape
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    scale = torch.empty_like(mean)
    shift = torch.empty_like(mean)
    ws = _ws(B, C, L, 3, 0, x.device)
    check(_lib.load().segan_bn_stats(_ptr(x), _ptr(gamma), _ptr(beta), eps, momentum,
                                     _ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(rstd),
                                     _ptr(scale), _ptr(shift), _ptr(ws), B, C, L, _stream()),
          'bn_stats')
    return mean, rstd, scale, shift


def bn_partial(x):
    """This rank's BatchNorm partial statistics ws[nsplit, C, 3] = (count, mean, M2)."""
    _chk(x, 'x', 3)
    B, C, L = x.shape
    ns = _lib.load().segan_bn_nsplit(B, C, L)
    ws = torch.empty((ns, C, 3), device=x.device, dtype=torch.float32)
    check(_lib.load().segan_bn_partial(_ptr(x), _ptr(ws), B, C, L, _stream()), 'bn_partial')
    return ws


def bn_final(ws_all, gamma, beta, eps, momentum, running_mean, running_var):
    """Combine partial statistics [nsplit_total, C, 3] (all ranks); returns (mean, rstd, scale,
    shift) and updates the running statistics like bn_stats."""
    _chk(ws_all, 'ws_all', 3)
    C = ws_all.shape[1]
    mean = torch.empty(C, device=ws_all.device, dtype=torch.float32)
    rstd, scale, shift = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
    check(_lib.load().segan_bn_final(_ptr(ws_all), ws_all.shape[0], _ptr(gamma), _ptr(beta), eps,
                                     momentum, _ptr(running_mean), _ptr(running_var), _ptr(mean),
                                     _ptr(rstd), _ptr(scale), _ptr(shift), C, _stream()), 'bn_final')
    return mean, rstd, scale, shift


def act_bwd_bn_reduce(a, dh, slope, bn, dslope=None, dgamma=None, dbeta=None):
    """First half of the BatchNorm backward: per-channel (sum g, sum g*xhat) of this rank's
    samples -> totals [C, 2]; accumulates dslope / dgamma / dbeta.  Returns (totals, ws)."""
    _chk(a, 'a', 3)
    B, C, L = a.shape
    mean, rstd, gamma, beta = bn
    totals = torch.empty((C, 2), device=a.device, dtype=torch.float32)
    ws = _ws(B, C, L, 4, 2, a.device)
    check(_lib.load().segan_act_bwd_bn_reduce(_ptr(a), _ptr(dh), _ptr(slope), _ptr(mean), _ptr(rstd),
                                              _ptr(gamma), _ptr(beta), _ptr(dslope), _ptr(dgamma),
                                              _ptr(dbeta), _ptr(totals), _ptr(ws), B, C, L, _stream()),
          'act_bwd_bn_reduce')
    return totals, ws


def act_bwd_bn_apply(a, dh, slope, bn, totals, count_total, dbias=None, ws=None):
    """Second half: da from the (globally summed) totals and the global element count."""
    _chk(a, 'a', 3)
    B, C, L = a.shape
    mean, rstd, gamma, beta = bn
    da = torch.empty_like(a)
    if ws is None:
        ws = _ws(B, C, L, 4, 2, a.device)
    check(_lib.load().segan_act_bwd_bn_apply(_ptr(a), _ptr(dh), _ptr(slope), _ptr(mean), _ptr(rstd),
                                             _ptr(gamma), _ptr(beta), _ptr(totals), _ptr(da),
                                             _ptr(dbias), _ptr(ws), B, C, L, float(count_total),
                                             _stream()), 'act_bwd_bn_apply')
    return da


def affine_prelu(x, scale=None, shift=None, slope=None):
    _chk(x, 'x', 3)
    B, C, L = x.shape
    y = torch.empty_like(x)
    check(_lib.load().segan_affine_prelu(_ptr(x), _ptr(scale), _ptr(shift), _ptr(slope), _ptr(y),
                                         B, C, L, _stream()), 'affine_prelu')
    return y


def affine_tanh(x, scale=None, shift=None):
    """tanh(x*scale + shift) with per-channel scale / shift on [B, C, L]."""
    _chk(x, 'x', 3)
    B, C, L = x.shape
    y = torch.empty_like(x)
    check(_lib.load().segan_affine_tanh(_ptr(x), _ptr(scale), _ptr(shift), _ptr(y), B, C, L,
                                        _stream()), 'affine_tanh')
    return y


def scale_mask(x, scale, mask):
    """x * scale[c] * mask on [B, C, L] (scale may be None): dropout on the skip path with the
    alpha scale folded in, and (scale None) its backward."""
    _chk(x, 'x', 3)
    _chk(mask, 'mask', 3)
    if mask.shape != x.shape:
        raise ValueError('scale_mask: mask {} vs x {}'.format(tuple(mask.shape), tuple(x.shape)))
    B, C, L = x.shape
    y = torch.empty_like(x)
    check(_lib.load().segan_scale_mask(_ptr(x), _ptr(scale), _ptr(mask), _ptr(y), B, C, L,
                                       _stream()), 'scale_mask')
    return y


def sum_skip(x0, slope0, x1, alpha):
    """prelu(x0, slope0) + alpha * x1 (GSkip merge_mode 'sum')."""
    _chk(x0, 'x0', 3)
    _chk(x1, 'x1', 3)
    if x0.shape != x1.shape:
        raise ValueError('sum_skip: shapes differ {} vs {}'.format(tuple(x0.shape), tuple(x1.shape)))
    B, C, L = x0.shape
    out = torch.empty_like(x0)
    check(_lib.load().segan_sum_skip(_ptr(x0), _ptr(slope0), _ptr(x1), _ptr(alpha), _ptr(out), B, C,
                                     L, _stream()), 'sum_skip')
    return out


def act_bwd(a, dh, dskip=None, slope=None, alpha=None, bn=None, dslope=None, dalpha=None,
            dgamma=None, dbeta=None, dbias=None):
    """Backward of (BN+)PReLU(+alpha skip) on pre-activation a; returns da.

    bn = (mean, rstd, gamma, beta) or None.  The d* tensors are accumulated into."""
    _chk(a, 'a', 3)
    B, C, L = a.shape
    da = torch.empty_like(a)
    ws = _ws(B, C, L, 4, 2, a.device)
    mean = rstd = gamma = beta = None
    if bn is not None:
        mean, rstd, gamma, beta = bn
    check(_lib.load().segan_act_bwd(_ptr(a), _ptr(dh), _ptr(dskip), _ptr(slope), _ptr(alpha),
                                    _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(da),
                                    _ptr(dslope), _ptr(dalpha), _ptr(dgamma), _ptr(dbeta),
                                    _ptr(dbias), _ptr(ws), B, C, L, _stream()), 'act_bwd')
    return da


def tanh_bwd(y, dy, clean=None, l1_scale=0.0, dbias=None):
    _chk(y, 'y', 3)
    B, C, L = y.shape
    da = torch.empty_like(y)
    ws = _ws(B, C, L, 1, 0, y.device)
    check(_lib.load().segan_tanh_bwd(_ptr(y), _ptr(dy), _ptr(clean), float(l1_scale), _ptr(da),
                                     _ptr(dbias), _ptr(ws), B, C, L, _stream()), 'tanh_bwd')
    return da


# ---------------------------------------------------------------------------------
# dense head
# ---------------------------------------------------------------------------------
def gemm(A, sam, sak, Bm, sbk, sbn, C, M, N, K, overwrite):
    lib = _lib.load()
    sp, sn = None, 0
    if _deterministic:      # split-K partials as slabs, added in split order
        sn = lib.segan_gemm_scratch_bytes(M, N, K)
        keep = torch.empty(sn, device=C.device, dtype=torch.uint8)
        sp = ctypes.c_void_p(keep.data_ptr())
    check(lib.segan_gemm(_ptr(A), sam, sak, _ptr(Bm), sbk, sbn, _ptr(C), C.stride(0), M, N,
                         K, 1 if overwrite else 0, 1 if _deterministic else 0, sp, sn, _stream()),
          'gemm')


def linear_fwd(x, w):
    """x [B, I] @ w[O, I]^T -> [B, O] (no bias)."""
    _chk(x, 'x', 2)
    _chk(w, 'w', 2)
    Bn, I = x.shape
    O = w.shape[0]
    y = torch.empty((Bn, O), device=x.device, dtype=torch.float32)
    gemm(x, I, 1, w, 1, I, y, Bn, O, I, True)
    return y


def linear_dgrad(dy, w):
    """dy [B, O] @ w[O, I] -> [B, I]."""
    Bn, O = dy.shape
    I = w.shape[1]
    dx = torch.empty((Bn, I), device=dy.device, dtype=torch.float32)
    gemm(dy, O, 1, w, I, 1, dx, Bn, I, O, True)
    return dx


def linear_wgrad(dy, x, dw):
    """dw[O, I] += dy[B, O]^T @ x[B, I]."""
    Bn, O = dy.shape
    I = x.shape[1]
    gemm(dy, 1, O, x, I, 1, dw, O, I, Bn, False)


def bias_prelu_rows(x, bias, slope):
    _chk(x, 'x', 2)
    y = torch.empty_like(x)
    check(_lib.load().segan_bias_prelu_rows(_ptr(x), _ptr(bias), _ptr(slope), _ptr(y), x.shape[0],
                                            x.shape[1], _stream()), 'bias_prelu_rows')
    return y


def bias_prelu_rows_bwd(x, bias, slope, dy, dslope, dbias):
    dx = torch.empty_like(x)
    check(_lib.load().segan_bias_prelu_rows_bwd(_ptr(x), _ptr(bias), _ptr(slope), _ptr(dy),
                                                _ptr(dx), _ptr(dslope), _ptr(dbias), x.shape[0],
                                                x.shape[1], _stream()), 'bias_prelu_rows_bwd')
    return dx


# ---------------------------------------------------------------------------------
# losses / optimizers / utilities
# ---------------------------------------------------------------------------------
def pool_time_fwd(x, mode):
    """Global pooling over time of x [B, C, L] -> ([B, C], idx): mode 'max' (idx = first argmax,
    int32 [B, C]) or 'avg' (idx None).  AdaptiveMaxPool1d(1) / AdaptiveAvgPool1d(1) of the
    'gmax' / 'gavg' discriminator heads (discriminator.py:128-137)."""
    _chk(x, 'x', 3)
    B, C, L = x.shape
    y = torch.empty((B, C), device=x.device, dtype=torch.float32)
    idx = torch.empty((B, C), device=x.device, dtype=torch.int32) if mode == 'max' else None
    check(_lib.load().segan_pool_time_fwd(_ptr(x), _ptr(y), _ptr(idx), B * C, L,
                                          0 if mode == 'max' else 1, _stream()), 'pool_time_fwd')
    return y, idx


def pool_time_bwd(dy, idx, L, mode):
    """Gradient of pool_time_fwd w.r.t. x: [B, C, L]."""
    _chk(dy, 'dy', 2)
    B, C = dy.shape
    dx = torch.empty((B, C, L), device=dy.device, dtype=torch.float32)
    check(_lib.load().segan_pool_time_bwd(_ptr(dy), _ptr(idx), _ptr(dx), B * C, L,
                                          0 if mode == 'max' else 1, _stream()), 'pool_time_bwd')
    return dx


def mse_const(x, target):
    """mean((x - target)^2) for a constant target (LSGAN labels, model.py:298,305,316)."""
    _chk(x, 'x')
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    check(_lib.load().segan_mse_const(_ptr(x), float(target), _ptr(loss), None, None, 1.0,
                                      x.numel(), _stream()), 'mse_const')
    return loss


def mse_const_bwd(x, target, gout=None, gscale=1.0):
    """Gradient of mse_const times the (device-resident) upstream scalar gout."""
    _chk(x, 'x')
    grad = torch.empty_like(x)
    check(_lib.load().segan_mse_const(_ptr(x), float(target), None, _ptr(grad), _ptr(gout),
                                      float(gscale), x.numel(), _stream()), 'mse_const_bwd')
    return grad


def bce_logits_const(x, target):
    _chk(x, 'x')
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    check(_lib.load().segan_bce_logits_const(_ptr(x), float(target), _ptr(loss), None, None, 1.0,
                                             x.numel(), _stream()), 'bce_logits_const')
    return loss


def bce_logits_const_bwd(x, target, gout=None, gscale=1.0):
    _chk(x, 'x')
    grad = torch.empty_like(x)
    check(_lib.load().segan_bce_logits_const(_ptr(x), float(target), None, _ptr(grad), _ptr(gout),
                                             float(gscale), x.numel(), _stream()),
          'bce_logits_const_bwd')
    return grad


def l1_bwd(x, y, gout=None, gscale=1.0):
    _chk(x, 'x')
    grad = torch.empty_like(x)
    check(_lib.load().segan_l1_bwd(_ptr(x), _ptr(y), _ptr(gout), float(gscale), _ptr(grad),
                                   x.numel(), _stream()), 'l1_bwd')
    return grad


def l1_mean(x, y):
    _chk(x, 'x')
    _chk(y, 'y')
    if x.shape != y.shape:
        raise ValueError('l1_mean: shapes differ {} vs {}'.format(tuple(x.shape), tuple(y.shape)))
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    ws = torch.empty(1024, device=x.device, dtype=torch.float32)
    check(_lib.load().segan_l1_mean(_ptr(x), _ptr(y), _ptr(loss), _ptr(ws), x.numel(), _stream()),
          'l1_mean')
    return loss


def mse_mean(x, y):
    """mean((x - y)^2) of two tensors (F.mse_loss; --reg_loss mse_loss)."""
    _chk(x, 'x')
    _chk(y, 'y')
    if x.shape != y.shape:
        raise ValueError('mse_mean: shapes differ {} vs {}'.format(tuple(x.shape), tuple(y.shape)))
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    ws = torch.empty(1024, device=x.device, dtype=torch.float32)
    check(_lib.load().segan_mse_mean(_ptr(x), _ptr(y), _ptr(loss), _ptr(ws), x.numel(), _stream()),
          'mse_mean')
    return loss


def mse_bwd(x, y, gout=None, gscale=1.0):
    _chk(x, 'x')
    grad = torch.empty_like(x)
    check(_lib.load().segan_mse_bwd(_ptr(x), _ptr(y), _ptr(gout), float(gscale), _ptr(grad),
                                    x.numel(), _stream()), 'mse_bwd')
    return grad


# ---- STFT power loss (model.py:640-653) ----------------------------------------------------
_stft_basis_cache = {}


def stft_pitch(n_fft):
    """Row width of the basis / spectra: 2*(n_fft/2+1) rounded up to a multiple of 4."""
    return (2 * (n_fft // 2 + 1) + 3) // 4 * 4


def stft_basis(n_fft, win, device):
    """[win, pitch] real DFT basis of a centred rectangular window (cached): columns
    [0, nbins) real part, [nbins, 2*nbins) imaginary part, zero padding up to the pitch."""
    key = (n_fft, win, str(device))
    if key not in _stft_basis_cache:
        bs = torch.empty((win, stft_pitch(n_fft)), device=device, dtype=torch.float32)
        check(_lib.load().segan_stft_basis(_ptr(bs), n_fft, win, _stream()), 'stft_basis')
        _stft_basis_cache[key] = bs
    return _stft_basis_cache[key]


def _stft_even(n_fft, what):
    # one reflection reaches 2(T-1); an odd n_fft can ask for one sample more, and its frame
    # count is not torch.stft's when hop divides T (segan_stft.hip refuses it as well)
    if n_fft % 2:
        raise ValueError('{}: odd n_fft={} is not supported (n_fft must be even)'.format(what, n_fft))


def stft_frames(x, n_fft, hop, win):
    """x [B, T] -> frames [B*NF, win] of the reflect-padded signal (even n_fft, n_fft/2 < T)."""
    _chk(x, 'x', 2)
    _stft_even(n_fft, 'stft_frames')
    B, T = x.shape
    NF = 1 + T // hop
    fr = torch.empty((B * NF, win), device=x.device, dtype=torch.float32)
    check(_lib.load().segan_stft_frames(_ptr(x), _ptr(fr), B, T, n_fft, hop, win, _stream()),
          'stft_frames')
    return fr


def stft_spectrum(frames, basis):
    """frames [R, win] @ basis [win, pitch] -> [R, pitch] (real | imaginary | zero pad)."""
    R, win = frames.shape
    N2 = basis.shape[1]
    S = torch.empty((R, N2), device=frames.device, dtype=torch.float32)
    gemm(frames, win, 1, basis, N2, 1, S, R, N2, win, True)
    return S


def stft_spectrum_bwd(dS, basis):
    """dS [R, pitch] @ basis^T -> dframes [R, win]."""
    R, N2 = dS.shape
    win = basis.shape[0]
    df = torch.empty((R, win), device=dS.device, dtype=torch.float32)
    gemm(dS, N2, 1, basis, 1, N2, df, R, win, N2, True)
    return df


def powdb(S, nbins, eps=10e-20):
    _chk(S, 'S', 2)
    rows, pitch = S.shape
    db = torch.empty((rows, nbins), device=S.device, dtype=torch.float32)
    check(_lib.load().segan_powdb(_ptr(S), _ptr(db), rows, nbins, pitch, eps, _stream()), 'powdb')
    return db


def powdb_bwd(S, ddb, nbins, eps=10e-20):
    _chk(S, 'S', 2)
    _chk(ddb, 'ddb', 2)
    rows, pitch = S.shape
    dS = torch.empty_like(S)
    check(_lib.load().segan_powdb_bwd(_ptr(S), _ptr(ddb), _ptr(dS), rows, nbins, pitch, eps,
                                      _stream()), 'powdb_bwd')
    return dS


def stft_overlap_add(dframes, B, T, n_fft, hop, win):
    _chk(dframes, 'dframes', 2)
    _stft_even(n_fft, 'stft_overlap_add')
    dx = torch.empty((B, T), device=dframes.device, dtype=torch.float32)
    check(_lib.load().segan_stft_overlap_add(_ptr(dframes), _ptr(dx), B, T, n_fft, hop, win,
                                             _stream()), 'stft_overlap_add')
    return dx


# ---- spectral normalisation -----------------------------------------------------------------
def _sn_view(w, dim):
    """[A, Bd, K] view of a weight for the C ABI: Conv1d / ConvTranspose1d [A, Bd, K], Linear
    [A, Bd] (K = 1), PReLU [A] (Bd = K = 1)."""
    shp = tuple(w.shape) + (1,) * (3 - w.dim())
    if w.dim() > 3 or dim not in (0, 1) or (dim == 1 and w.dim() < 2):
        raise ValueError('snorm: unsupported weight shape {} / dim {}'.format(tuple(w.shape), dim))
    return shp


def snorm_fwd(w, u, v, dim, power_iteration, eps=1e-12):
    """(w / sigma, sigma) of torch.nn.utils.spectral_norm; u, v are updated in place when
    `power_iteration` (training mode)."""
    _chk(w, 'w')
    _chk(u, 'u', 1)
    _chk(v, 'v', 1)
    A, Bd, K = _sn_view(w, dim)
    rows, cols = (A, Bd * K) if dim == 0 else (Bd, A * K)
    if u.numel() != rows or v.numel() != cols:
        raise ValueError('snorm: u[{}] / v[{}] do not match the {}x{} matrix view'.format(
            u.numel(), v.numel(), rows, cols))
    lib = _lib.load()
    w_sn = torch.empty_like(w)
    sigma = torch.empty(1, device=w.device, dtype=torch.float32)
    ws = torch.empty(lib.segan_snorm_ws_floats(A, Bd, K, dim), device=w.device, dtype=torch.float32)
    check(lib.segan_snorm_fwd(_ptr(w), _ptr(u), _ptr(v), _ptr(w_sn), _ptr(sigma), _ptr(ws), A, Bd, K,
                              dim, 1 if power_iteration else 0, float(eps), _stream()), 'snorm_fwd')
    return w_sn, sigma


def snorm_bwd(dw_sn, w, u, v, sigma, dim, dw):
    """dw += d(w/sigma)^T dw_sn with u, v held constant (how torch differentiates it)."""
    _chk(dw_sn, 'dw_sn')
    _chk(dw, 'dw')
    A, Bd, K = _sn_view(w, dim)
    lib = _lib.load()
    ws = torch.empty(lib.segan_snorm_ws_floats(A, Bd, K, dim), device=w.device, dtype=torch.float32)
    check(lib.segan_snorm_bwd(_ptr(dw_sn), _ptr(w), _ptr(u), _ptr(v), _ptr(sigma), _ptr(dw), _ptr(ws),
                              A, Bd, K, dim, _stream()), 'snorm_bwd')


def pcm16_prep(pcm, first, coef):
    """int16 slices [B, 2, T+1] (+ first[B] uint8) -> (clean, noisy) fp32 [B, T]: min-max
    normalisation and pre-emphasis of se_dataset.py:108-117 on the GPU, bit-exact."""
    if pcm.dtype != torch.int16 or first.dtype != torch.uint8 or not pcm.is_cuda or not first.is_cuda:
        raise TypeError('pcm16_prep: pcm must be a CUDA int16 tensor and first a CUDA uint8 tensor')
    if pcm.dim() != 3 or pcm.shape[1] != 2 or not pcm.is_contiguous() or first.numel() != pcm.shape[0]:
        raise ValueError('pcm16_prep: pcm must be contiguous [B, 2, T+1], first [B]')
    B, T = pcm.shape[0], pcm.shape[2] - 1
    clean = torch.empty((B, T), device=pcm.device, dtype=torch.float32)
    noisy = torch.empty((B, T), device=pcm.device, dtype=torch.float32)
    check(_lib.load().segan_pcm16_prep(ctypes.c_void_p(pcm.data_ptr()),
                                       ctypes.c_void_p(first.data_ptr()), _ptr(clean), _ptr(noisy),
                                       B, T, float(coef), _stream()), 'pcm16_prep')
    return clean, noisy


def de_emphasize(y, coef):
    """x[n] = coef*x[n-1] + y[n] along the last axis of a CUDA tensor [..., T] (se_dataset.py:
    119-126 on the device)."""
    _chk(y, 'y')
    T = y.shape[-1]
    x = torch.empty_like(y)
    check(_lib.load().segan_deemphasis(_ptr(y), _ptr(x), y.numel() // T, T, float(coef), _stream()),
          'deemphasis')
    return x


def ssnr(ref, deg, srate=16000, eps=1e-10):
    """Segmental SNR of utils.py:350-395 per row of ref / deg [rows, T] on the device.  Returns
    (overall_snr[rows], mean_segmental_snr[rows], segmental[rows, nframes])."""
    rows, T = _chk_pair('ssnr', ref, deg)
    lib = _lib.load()
    nf = lib.segan_ssnr_frames(T, srate)
    seg = torch.empty((rows, max(nf, 1)), device=ref.device, dtype=torch.float32)
    out = torch.empty((rows, 2), device=ref.device, dtype=torch.float32)
    check(lib.segan_ssnr(_ptr(ref), _ptr(deg), _ptr(seg), _ptr(out), rows, T, srate, float(eps),
                         _stream()), 'ssnr')
    return out[:, 0], out[:, 1], seg[:, :nf]


def _quality_frames(fn, what, ref, deg, srate):
    rows, T = _chk_pair(what, ref, deg)
    nf = _lib.load().segan_ssnr_frames(T, srate)
    dist = torch.empty((rows, max(nf, 1)), device=ref.device, dtype=torch.float64)
    check(fn(_ptr(ref), _ptr(deg), _ptr(dist), rows, T, srate, _stream()), what)
    return dist[:, :nf]


def wss(ref, deg, srate=16000):
    """Per-frame weighted spectral slope distortion of utils.py:442-596 for the rows of ref / deg
    [rows, T] on the device: fp64 [rows, nframes] (the SSNR frames)."""
    return _quality_frames(_lib.load().segan_wss, 'wss', ref, deg, srate)


def llr(ref, deg, srate=16000):
    """Per-frame log-likelihood ratio of utils.py:598-716 for the rows of ref / deg [rows, T] on
    the device: fp64 [rows, nframes]; NaN where the clean frame is all zeros."""
    return _quality_frames(_lib.load().segan_llr, 'llr', ref, deg, srate)


STOI_SRATES = (4000, 48000)
STOI_BANDS = 15


def _int_arg(v, what, lo, hi):
    try:
        out = None if isinstance(v, bool) else operator.index(v)
    except TypeError:
        out = None
    if out is None or not lo <= out <= hi:
        raise ValueError('{} must be an integer from {} to {}, got {!r}'.format(what, lo, hi, v))
    return out


def _fetch_taps(plan, what):
    """The two calls of a segan_*_plan entry: plan(pq, ntaps, taps, cap) once without a buffer for
    the count, once with one.  Returns (p, q, fp64 CPU taps)."""
    pq, n = (ctypes.c_int * 2)(), ctypes.c_int()
    check(plan(pq, ctypes.byref(n), None, 0), what)
    taps = torch.empty(n.value, dtype=torch.float64)
    check(plan(pq, ctypes.byref(n), _ptr(taps), n.value), what)
    return pq[0], pq[1], taps


def stoi_plan(srate):
    """The host-side plan of STOI at `srate` (no device involved): (p, q, taps, bands) with p / q
    = 10000 / srate in lowest terms, the fp64 CPU tensor of 20 max(p, q) + 1 resampling taps and
    the int CPU tensor [15, 2] of each third-octave band's DFT bins [lo, hi)."""
    srate = _int_arg(srate, 'stoi: srate', *STOI_SRATES)
    lib = _lib.load()
    bands = (ctypes.c_int * (2 * STOI_BANDS))()
    p, q, taps = _fetch_taps(lambda *a: lib.segan_stoi_plan(srate, *a, bands), 'stoi_plan')
    return p, q, taps, torch.tensor(list(bands), dtype=torch.int64).view(STOI_BANDS, 2)


def _row_lengths(what, lengths, rows, T, device, device_ok=False):
    """Host integers [rows], checked to lie in 0 .. T, as an int32 tensor on `device`.  With
    `device_ok`, a CUDA tensor is used as it is (int32 [rows] on `device`; its values are left to
    the kernel) and nothing is copied to the host."""
    if device_ok and isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or lengths.shape != (rows,) or lengths.device != device:
            raise ValueError('{}: device lengths must be int32 [{}] on {}'.format(what, rows, device))
        return lengths.contiguous()
    lens = torch.as_tensor(lengths).detach().cpu()
    if lens.dim() != 1 or lens.numel() != rows or lens.dtype.is_floating_point or lens.dtype in (
            torch.bool, torch.complex64, torch.complex128):
        raise ValueError('{}: lengths must hold {} integers, got {}'.format(what, rows, lengths))
    if rows and (int(lens.min()) < 0 or int(lens.max()) > T):
        raise ValueError('{}: lengths must lie in 0 .. {}, got {}'.format(what, T, lens.tolist()))
    return lens.to(dtype=torch.int32).to(device)


def _stoi_run(entry, last, per, ref, deg, srate, lengths):
    """The argument checks, stage buffers and call that segan_stoi and segan_estoi share: `entry`
    names the C entry, `last` its last-stage buffer ([rows, S, per], [rows, S] with per = 1)."""
    rows, T = _chk_pair('stoi', ref, deg)
    srate = _int_arg(srate, 'stoi: srate', *STOI_SRATES)
    lens = None if lengths is None else _row_lengths('stoi', lengths, rows, T, ref.device)
    lib = _lib.load()
    dims = (ctypes.c_int * 5)()
    check(lib.segan_stoi_dims(T, srate, dims), 'stoi')
    Ly, F, Lc, Fb, S = list(dims)
    f64 = dict(device=ref.device, dtype=torch.float64)
    i32 = dict(device=ref.device, dtype=torch.int32)
    xr = torch.empty((2, rows, max(Ly, 1)), **f64)
    energy = torch.empty((rows, max(F, 1)), **f64)
    mask = torch.empty((rows, max(F, 1)), **i32)
    kept = torch.empty((rows, max(F, 1)), **i32)
    count = torch.empty(rows, **i32)
    xs = torch.empty((2, rows, max(Lc, 1)), **f64)
    env = torch.empty((2, rows, STOI_BANDS, max(Fb, 1)), **f64)
    seg = torch.empty((rows, max(S, 1)) + ((per,) if per > 1 else ()), **f64)
    d = torch.empty(rows, **f64)
    check(getattr(lib, 'segan_' + entry)(
        _ptr(ref), _ptr(deg), _ptr(lens), rows, T, srate, _ptr(xr[0]), _ptr(xr[1]), _ptr(energy),
        _ptr(mask), _ptr(kept), _ptr(count), _ptr(xs[0]), _ptr(xs[1]), _ptr(env[0]), _ptr(env[1]),
        _ptr(seg), _ptr(d), _stream()), entry)
    out = dict(xr=xr[0, :, :Ly], yr=xr[1, :, :Ly], energy=energy[:, :F], mask=mask[:, :F],
               kept=kept[:, :F], count=count, xs=xs[0, :, :Lc], ys=xs[1, :, :Lc],
               X=env[0, :, :, :Fb], Y=env[1, :, :, :Fb], d=d, dims=(Ly, F, Lc, Fb, S))
    out[last] = seg[:, :S]
    return out


def stoi_stages(ref, deg, srate=16000, lengths=None):
    """STOI (Taal et al.'s short-time objective intelligibility) of each
    row of ref / deg [rows, T] with every intermediate, fp64, on the device.  Row r is the signal
    ref[r, :lengths[r]] (all T without `lengths`; host integers, a CUDA tensor is copied to the
    host to be checked).  Returns a dict of device tensors, sized for T, of which each row uses
    its own leading part: xr, yr [rows, Ly] (resampled to 10 kHz), energy, mask, kept
    [rows, F] (clean frame energies in dB, keep mask, kept frame indices), count [rows] (M),
    xs, ys [rows, Lc] (compacted), X, Y [rows, 15, Fb] (band envelopes), rho [rows, S, 15]
    (segment correlations), d [rows]; and dims = (Ly, F, Lc, Fb, S)."""
    return _stoi_run('stoi', 'rho', STOI_BANDS, ref, deg, srate, lengths)


def stoi(ref, deg, srate=16000, lengths=None):
    """STOI of each row of ref / deg [rows, T] (fp32 CUDA tensors) on the device: fp64 [rows],
    NaN where it is undefined (a clean signal of digital silence, fewer than 30 band frames after
    silent-frame removal, a 0/0 correlation).  `lengths`: optional per-row valid sample counts
    (see stoi_stages).  srate: any integer from 4000 to 48000 Hz.  No device-to-host copy."""
    return stoi_stages(ref, deg, srate, lengths)['d']


def estoi_stages(ref, deg, srate=16000, lengths=None):
    """ESTOI (Jensen & Taal's extended STOI) of each row of ref / deg
    [rows, T] with every intermediate: stoi_stages' dict (the same arguments, checks and stages
    up to the band envelopes X, Y) with dm [rows, S], each segment's normalised-window inner
    product / 30, in place of rho, and d [rows] their mean."""
    return _stoi_run('estoi', 'dm', 1, ref, deg, srate, lengths)


def estoi(ref, deg, srate=16000, lengths=None):
    """ESTOI of each row of ref / deg [rows, T] (fp32 CUDA tensors) on the device: fp64 [rows],
    NaN where it is undefined (a clean signal of digital silence, fewer than 30 band frames after
    silent-frame removal).  Arguments as for `stoi`.  No device-to-host copy."""
    return estoi_stages(ref, deg, srate, lengths)['d']


SISDR_SPAN = _D['SEGAN_SISDR_SPAN']      # samples per partial sum


def _measure_args(what, ref, deg, lengths):
    """The argument checks of ops.stoi for the measures with per-row lengths: fp32 CUDA [rows, T]
    of one shape, host integers 1 <= lengths[r] <= T.  Returns (rows, T, device int32 lengths or
    None)."""
    rows, T = _chk_pair(what, ref, deg)
    if rows < 1 or T < 1:
        raise ValueError('{}: empty input {}'.format(what, tuple(ref.shape)))
    lens = None
    if lengths is not None:
        host = torch.as_tensor(lengths).detach().cpu()
        lens = _row_lengths(what, host, rows, T, ref.device)
        if int(host.min()) < 1:
            raise ValueError('{}: lengths must lie in 1 .. {}, got {}'.format(what, T, host.tolist()))
    return rows, T, lens


def _measure_srate(what, srate):
    return _int_arg(srate, what + ': srate', 1, 1 << 20)


def fwsegsnr(ref, deg, srate=16000, lengths=None):
    """Frequency-weighted segmental SNR (Hu & Loizou's fwSNRseg) of each row
    of ref / deg [rows, T] (fp32 CUDA tensors) on the device, on the frames of `wss`.  Row r is
    ref[r, :lengths[r]] (all T without `lengths`; host integers as in `stoi`).  Returns (frames
    [rows, nframes] fp64, clipped to [-10, 35], NaN where a frame of either signal is digital
    silence and past the row's own frame count; value [rows] fp64, the mean of the row's finite
    frames, NaN without any).  No device-to-host copy."""
    rows, T, lens = _measure_args('fwsegsnr', ref, deg, lengths)
    srate = _measure_srate('fwsegsnr', srate)
    lib = _lib.load()
    nf = lib.segan_ssnr_frames(T, srate)
    frames = torch.empty((rows, max(nf, 1)), device=ref.device, dtype=torch.float64)
    value = torch.empty(rows, device=ref.device, dtype=torch.float64)
    check(lib.segan_fwsegsnr(_ptr(ref), _ptr(deg), _ptr(lens), rows, T, srate, _ptr(frames),
                             _ptr(value), _stream()), 'fwsegsnr')
    return frames[:, :nf], value


def cepstral_distance(ref, deg, srate=16000, lengths=None):
    """Per-frame LPC cepstrum distance (Hu & Loizou's CD) of each row of
    ref / deg [rows, T] on the device, on the frames and lags of `llr` with an fp64 Levinson
    recursion: fp64 [rows, nframes], at most 10, NaN where a frame of either signal has no energy
    and past the row's own frame count.  `lengths` as in `fwsegsnr`."""
    rows, T, lens = _measure_args('cepstral_distance', ref, deg, lengths)
    srate = _measure_srate('cepstral_distance', srate)
    lib = _lib.load()
    nf = lib.segan_ssnr_frames(T, srate)
    frames = torch.empty((rows, max(nf, 1)), device=ref.device, dtype=torch.float64)
    check(lib.segan_cepdist(_ptr(ref), _ptr(deg), _ptr(lens), rows, T, srate, _ptr(frames),
                            _stream()), 'cepstral_distance')
    return frames[:, :nf]


def si_sdr(ref, deg, lengths=None):
    """Scale-invariant SDR (Le Roux et al. 2019) in dB of each row of ref / deg [rows, T] on the
    device: fp64 [rows]; NaN where the clean row (mean removed) has no energy, +inf where the
    processed row is a scaled and shifted copy of it to the last bit.  Fixed summation order: two
    calls return the same bits.  `lengths` as in `fwsegsnr`.  No device-to-host copy."""
    rows, T, lens = _measure_args('si_sdr', ref, deg, lengths)
    out = torch.empty(rows, device=ref.device, dtype=torch.float64)
    ws = torch.empty(rows * (4 * ((T + SISDR_SPAN - 1) // SISDR_SPAN) + 4), device=ref.device,
                     dtype=torch.float64)
    check(_lib.load().segan_sisdr(_ptr(ref), _ptr(deg), _ptr(lens), rows, T, _ptr(out), _ptr(ws),
                                  _stream()), 'si_sdr')
    return out


SDR_TAPS = _D['SEGAN_SDR_MAX_TAPS']      # the longest distortion filter
SDR_SPAN = _D['SEGAN_SDR_SPAN']          # samples per partial sum


def sdr_stages(ref, deg, lengths=None, taps=SDR_TAPS):
    """Every stage of `sdr` (BSS-eval SDR) of each row of ref / deg
    [rows, T] (fp32 CUDA tensors) on the device, as a dict of fp64 tensors: 'r', 'd' [rows, taps]
    (the lagged auto- and cross-correlations), 'c' [rows, taps] (the distortion filter, zero from
    the order reached on), 'order' [rows] (int64: taps unless the recursion's guard stopped it),
    'target_energy', 'error_energy', 'sdr' [rows].  Row r is ref[r, :lengths[r]] (host integers
    0 .. T; all T without `lengths`).  No device-to-host copy."""
    rows, T = _chk_pair('sdr', ref, deg)
    if not 1 <= rows <= 65535 or T < 1:
        raise ValueError('sdr: 1 .. 65535 rows of at least one sample, got {}'.format(
            tuple(ref.shape)))
    n = _int_arg(taps, 'sdr: taps', 1, SDR_TAPS)
    lens = None if lengths is None else _row_lengths('sdr', lengths, rows, T, ref.device)
    lib = _lib.load()
    dims = (ctypes.c_int64 * 3)()
    check(lib.segan_sdr_dims(rows, T, n, dims), 'sdr')
    ws = _stream_scratch(8 * dims[2], ref.device)
    out = torch.empty(rows, device=ref.device, dtype=torch.float64)
    stages = torch.empty((rows, 3 * n + 3), device=ref.device, dtype=torch.float64)
    check(lib.segan_sdr(_ptr(ref), _ptr(deg), _ptr(lens), rows, T, n, _ptr(out), _ptr(stages),
                        _ptr(ws), _stream()), 'sdr')
    return {'r': stages[:, :n], 'd': stages[:, n:2 * n], 'c': stages[:, 2 * n:3 * n],
            'order': stages[:, 3 * n].to(torch.int64), 'target_energy': stages[:, 3 * n + 1],
            'error_energy': stages[:, 3 * n + 2], 'sdr': out}


def sdr(ref, deg, lengths=None, taps=SDR_TAPS):
    """BSS-eval signal-to-distortion ratio in dB (the SDR of bss_eval_sources) of each row of
    ref / deg [rows, T] on the device: deg is projected onto the span of ref and its first
    taps - 1 delays (taps in 1 .. 512), 10 log10 of the projection's energy over the rest's; fp64
    [rows].  NaN for a row of no samples, a clean row without energy or a processed row of zeros;
    +inf where the processed row is the clean one times a power of two.  Fixed summation order: a
    batched row equals its own call bit for bit.  `lengths` as in `sdr_stages`."""
    return sdr_stages(ref, deg, lengths, taps)['sdr']


def toeplitz_solve(r, d):
    """Solves Toeplitz(r) c = d for each row of r / d ([rows, n] or [n] fp64 CUDA tensors, n <=
    512; r the first column of a symmetric positive definite Toeplitz matrix) by the Levinson
    recursion on the device.  Returns (c fp64 like r, order int32 [rows]): at order m with
    prediction error E_m <= 2^-40 r[0] the recursion stops, c[m:] is zero and order is m; else
    order is n."""
    _chk(r, 'r', dtype=torch.float64, contiguous=False)
    _chk(d, 'd', dtype=torch.float64, contiguous=False)
    if r.shape != d.shape or r.dim() not in (1, 2):
        raise ValueError('toeplitz_solve: r {} and d {} must be [rows, n] or [n] of one shape'
                         .format(tuple(r.shape), tuple(d.shape)))
    r2, d2 = r.reshape(-1, r.shape[-1]).contiguous(), d.reshape(-1, r.shape[-1]).contiguous()
    rows, n = r2.shape
    if not 1 <= rows <= 65535 or not 1 <= n <= SDR_TAPS:
        raise ValueError('toeplitz_solve: 1 .. 65535 rows of 1 .. {} values, got {}'.format(
            SDR_TAPS, tuple(r.shape)))
    c = torch.empty_like(r2)
    order = torch.empty(rows, device=r.device, dtype=torch.int32)
    check(_lib.load().segan_toeplitz_solve(_ptr(r2), _ptr(d2), rows, n, _ptr(c), _ptr(order),
                                           _stream()), 'toeplitz_solve')
    return c.reshape(r.shape), order


FFT_MAX_LOG2 = _D['SEGAN_FFT_MAX_LOG2']      # the longest transform, 2^20
FFT_LDS_LOG2 = _D['SEGAN_FFT_LDS_LOG2']      # up to 2^12 points one workgroup transforms in LDS
SRMR_CHANNELS = _D['SEGAN_SRMR_CHANNELS']    # gammatone channels
SRMR_BANDS = _D['SEGAN_SRMR_BANDS']          # modulation bands
SRMR_STAGE = _D['SEGAN_SRMR_STAGE']          # doubles of one row's stage block
SRMR_RATES = (8000, 16000)
SRMR_WS_CAP = 1 << 30    # bytes of workspace one call of segan_srmr may take


def fft_pow2(x, inverse=False):
    """The discrete Fourier transform of each row of x ([rows, n] or [n] complex128 CUDA tensor,
    n a power of two from 2 to 2^20) on the device, numpy.fft.fft's sign and scaling
    (`inverse=True`: numpy.fft.ifft's, with 1/n).  Up to n = 4096 one workgroup transforms a row
    in LDS; above that the transform runs as two levels.  Returns a new tensor like x."""
    _chk(x, 'x', dtype=torch.complex128, contiguous=False)
    if x.dim() not in (1, 2):
        raise ValueError('fft_pow2: x must be [rows, n] or [n], got {}'.format(tuple(x.shape)))
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    rows, n = x2.shape
    lg = n.bit_length() - 1
    if not 1 <= rows <= 65535 or n < 2 or n != 1 << lg or lg > FFT_MAX_LOG2:
        raise ValueError('fft_pow2: 1 .. 65535 rows of a power of two from 2 to 2^{} values, got '
                         '{}'.format(FFT_MAX_LOG2, tuple(x.shape)))
    out = torch.empty_like(x2)
    check(_lib.load().segan_fft_z2z(_ptr(x2), _ptr(out), rows, lg, 1 if inverse else 0,
                                    _stream()), 'fft_pow2')
    return out.reshape(x.shape)


def srmr_stages(x, lengths=None, rate=16000, ws_cap=SRMR_WS_CAP):
    """Every stage of `srmr` of each row of x [rows, T] (fp32 CUDA tensor)
    on the device, as a dict of fp64 tensors: 'cfs' [23] (the gammatone centre frequencies,
    descending), 'envelope_energy' [rows, 23] (the sum of each channel's squared Hilbert envelope
    over the row's samples), 'energy' [rows, 23, 8] (the modulation energies, means over the
    frames), 'bw' [rows] (the ERB of the channel below which 90 % of the energy lies), 'kstar'
    [rows] (int64: 5 .. 8, the modulation bands counted; 0 for a NaN row), 'share' [rows] (the
    cumulated share in per cent that decided 'bw') and 'srmr' [rows].  Row r is x[r, :lengths[r]]
    (host integers 0 .. T; all T without `lengths`).  The rows are processed in chunks whose
    workspace stays under `ws_cap` bytes; the result is bit for bit the same for every chunking.
    No device-to-host copy."""
    _chk(x, 'x', 2)
    rows, T = x.shape
    if not 1 <= rows <= 65535 or not 1 <= T <= 1 << FFT_MAX_LOG2:
        raise ValueError('srmr: 1 .. 65535 rows of 1 .. 2^{} samples, got {}'.format(
            FFT_MAX_LOG2, tuple(x.shape)))
    if isinstance(rate, bool) or rate not in SRMR_RATES:
        raise ValueError('srmr: rate must be one of {}, got {!r}'.format(SRMR_RATES, rate))
    lens = None if lengths is None else _row_lengths('srmr', lengths, rows, T, x.device)
    lib = _lib.load()
    dims = (ctypes.c_int64 * 4)()
    check(lib.segan_srmr_dims(rows, T, rate, dims), 'srmr')
    cap = _int_arg(ws_cap, 'srmr: ws_cap', 1, 1 << 62)
    per = int(cap // (8 * dims[2]))
    if per < 1:
        raise ValueError('srmr: ws_cap of {} bytes is below the {} bytes one row of {} samples '
                         'needs'.format(cap, 8 * dims[2], T))
    per = min(per, rows)
    ws = _stream_scratch(8 * dims[2] * per + 16, x.device)
    ws = ws[(-ws.data_ptr()) % 16:]
    out = torch.empty(rows, device=x.device, dtype=torch.float64)
    stages = torch.empty((rows, SRMR_STAGE), device=x.device, dtype=torch.float64)
    for r0 in range(0, rows, per):
        n = min(per, rows - r0)
        check(lib.segan_srmr(_ptr(x[r0:r0 + n]), _ptr(None if lens is None else lens[r0:r0 + n]),
                             n, T, rate, _ptr(out[r0:r0 + n]), _ptr(stages[r0:r0 + n]), _ptr(ws),
                             _stream()), 'srmr')
    C, P = SRMR_CHANNELS, SRMR_CHANNELS * SRMR_BANDS
    return {'cfs': stages[0, :C], 'envelope_energy': stages[:, C:2 * C],
            'energy': stages[:, 2 * C:2 * C + P].reshape(rows, C, SRMR_BANDS),
            'bw': stages[:, 2 * C + P], 'kstar': stages[:, 2 * C + P + 1].to(torch.int64),
            'share': stages[:, 2 * C + P + 2], 'srmr': out}


def srmr(x, lengths=None, rate=16000, ws_cap=SRMR_WS_CAP):
    """SRMR, the speech-to-reverberation modulation energy ratio (Falk, Zheng and Chan 2010), of
    each row of x [rows, T] at `rate` (16000 or 8000) on the device: the energy of the envelope
    modulations below about 20 Hz, where speech lives, over that of the faster ones, which
    reverberation and noise fill; higher is better, and no clean signal is needed.  23 gammatone
    channels, 8 modulation bands, no energy normalisation; K*, the number of bands counted, is 5
    where the 90 % bandwidth lies at or below the fifth band's left cutoff, which the authors'
    toolbox leaves undefined.  fp64 [rows]; NaN for a row shorter than one frame of
    ceil(0.256 rate) samples or without energy.  Fixed operation order: a batched row equals its
    own call bit for bit, and a row times a power of two gives the same bits.  `lengths`,
    `ws_cap` as in `srmr_stages`."""
    return srmr_stages(x, lengths, rate, ws_cap)['srmr']


PITCH_NB = _D['SEGAN_PITCH_NB']      # hop blocks per frame
PITCH_RATES = (8000, 16000)
PITCH_THETA = 0.15       # YIN's threshold on the normalised difference
PITCH_MAX_T = 1 << 24
PITCH_WS_CAP = 1 << 30   # bytes of workspace one call of segan_pitch may take


def pitch_dims(rows, T, srate=16000):
    """segan_pitch_dims (host only) as a dict: hop, tau_min, tau_max, blocks and frames of a row
    of T samples, ws_doubles for `rows` rows."""
    dims = (ctypes.c_int64 * 6)()
    check(_lib.load().segan_pitch_dims(rows, T, srate, dims), 'pitch')
    return dict(zip(('hop', 'tau_min', 'tau_max', 'blocks', 'frames', 'ws_doubles'), list(dims)))


def _pitch_run(x, lengths, srate, threshold, ws_cap, want_cmnd):
    _chk(x, 'x', 2)
    rows, T = x.shape
    if not 1 <= rows <= 65535 or not 1 <= T <= PITCH_MAX_T:
        raise ValueError('pitch: 1 .. 65535 rows of 1 .. 2^24 samples, got {}'.format(
            tuple(x.shape)))
    if isinstance(srate, bool) or srate not in PITCH_RATES:
        raise ValueError('pitch: srate must be one of {}, got {!r}'.format(PITCH_RATES, srate))
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not (
            0 < threshold <= 1):
        raise ValueError('pitch: threshold must lie in (0, 1], got {!r}'.format(threshold))
    lens = None if lengths is None else _row_lengths('pitch', lengths, rows, T, x.device)
    cap = _int_arg(ws_cap, 'pitch: ws_cap', 1, 1 << 62)
    lib = _lib.load()
    d = pitch_dims(1, T, srate)
    F, nl = d['frames'], d['tau_max'] + 2
    per = int(cap // max(8 * d['ws_doubles'], 1))
    if per < 1:
        raise ValueError('pitch: ws_cap of {} bytes is below the {} bytes one row of {} samples '
                         'needs'.format(cap, 8 * d['ws_doubles'], T))
    per = min(per, rows)
    ws = _stream_scratch(max(8 * d['ws_doubles'] * per, 8), x.device)
    f64 = dict(device=x.device, dtype=torch.float64)
    f0 = torch.empty((rows, max(F, 1)), **f64)
    ap = torch.empty((rows, max(F, 1)), **f64)
    lag = torch.empty((rows, max(F, 1)), device=x.device, dtype=torch.int32)
    cm = torch.empty((rows, max(F, 1), nl), **f64) if want_cmnd else None
    for r0 in range(0, rows, per):
        n = min(per, rows - r0)
        xs, ls = x[r0:r0 + n], _ptr(None if lens is None else lens[r0:r0 + n])
        check(lib.segan_pitch(_ptr(xs), ls, n, T, srate, float(threshold), _ptr(f0[r0:r0 + n]),
                              _ptr(lag[r0:r0 + n]), _ptr(ap[r0:r0 + n]), _ptr(ws), _stream()),
              'pitch')
        if want_cmnd:
            check(lib.segan_pitch_cmnd(_ptr(xs), ls, n, T, srate, _ptr(cm[r0:r0 + n]), _ptr(ws),
                                       _stream()), 'pitch_cmnd')
    if lens is None:
        nframes = torch.full((rows,), F, device=x.device, dtype=torch.int32)
    else:
        host = lens.cpu().tolist()
        nframes = torch.tensor([lib.segan_pitch_frames(L, srate) for L in host],
                               dtype=torch.int32).to(x.device)
    out = {'f0': f0[:, :F], 'lag': lag[:, :F], 'ap': ap[:, :F], 'nframes': nframes}
    if want_cmnd:
        out['cmnd'] = cm[:, :F]
    return out


def pitch_stages(x, lengths=None, srate=16000, threshold=PITCH_THETA, ws_cap=PITCH_WS_CAP):
    """`pitch` with its intermediate as a dict of device tensors: 'f0',
    'lag', 'ap' [rows, F], 'nframes' [rows] (int32: each row's own frame count) and 'cmnd'
    [rows, F, tau_max + 2], YIN's cumulative-mean-normalised difference d' of every frame and lag
    (NaN from the row's own frame count on)."""
    return _pitch_run(x, lengths, srate, threshold, ws_cap, True)


def pitch(x, lengths=None, srate=16000, threshold=PITCH_THETA, ws_cap=PITCH_WS_CAP):
    """The pitch contour of each row of x [rows, T] (fp32 CUDA tensor) at `srate` (16000 or 8000)
    by YIN with a 5 ms hop on the device, fp64: (f0 [rows, F] in Hz, 0 when unvoiced; lag [rows, F]
    int32, the period picked in samples, 0 when unvoiced; ap [rows, F], d' at the pick or its
    minimum over the lag range when unvoiced; nframes [rows] int32).  A frame is 25 ms, lags run
    from srate / 400 to srate / 60.2; `threshold` in (0, 1].  Row r is x[r, :lengths[r]] (host
    integers 0 .. T; all T without `lengths`); frames from the row's own count on hold f0 = 0,
    lag = -1, ap = NaN.  The rows are processed in chunks whose workspace stays under `ws_cap`
    bytes.  Fixed operation order: a batched row equals its own call bit for bit, and a row times
    a power of two gives the same lags and f0 bits."""
    out = _pitch_run(x, lengths, srate, threshold, ws_cap, False)
    return out['f0'], out['lag'], out['ap'], out['nframes']


def f0_eval(f0_ref, lag_ref, f0_deg, lag_deg, nframes=None):
    """The F0 / voicing measures of the reference (ops.py:51-260 there) on the contours of a clean
    and a processed signal (`pitch`'s f0 fp64 and lag int32, [rows, F] CUDA tensors; `nframes`:
    int32 CUDA [rows], each row's frame count, all F without it): fp64 [rows, 4] = (f0_mae, the
    mean |f0 difference| in Hz over the clean contour's voiced frames; vuv_acc, the share of
    frames with the same voicing decision; f0_kld, the KL divergence between the Gaussian fits of
    the two log-f0 distributions; voiced, the clean contour's share of voiced frames), on the
    log-f0 contours interpolated linearly over the unvoiced frames.  NaN: all four without a
    frame; f0_mae and f0_kld where either contour has no voiced frame; f0_kld below two frames or
    for a constant processed contour."""
    _chk(f0_ref, 'f0_ref', 2, torch.float64)
    _chk(f0_deg, 'f0_deg', 2, torch.float64)
    _chk(lag_ref, 'lag_ref', 2, torch.int32)
    _chk(lag_deg, 'lag_deg', 2, torch.int32)
    if not f0_ref.shape == lag_ref.shape == f0_deg.shape == lag_deg.shape:
        raise ValueError('f0_eval: shapes differ: {}'.format(
            [tuple(t.shape) for t in (f0_ref, lag_ref, f0_deg, lag_deg)]))
    rows, F = f0_ref.shape
    if not 1 <= rows <= 65535:
        raise ValueError('f0_eval: 1 .. 65535 rows, got {}'.format(rows))
    if nframes is not None:
        _chk(nframes, 'nframes', 1, torch.int32)
        if nframes.shape != (rows,):
            raise ValueError('f0_eval: nframes must be int32 [{}]'.format(rows))
    out = torch.empty((rows, 4), device=f0_ref.device, dtype=torch.float64)
    if F == 0:      # an empty tensor has no address; the kernel reads nothing and writes NaN
        f0_ref = f0_deg = out
        lag_ref = lag_deg = torch.empty(1, device=out.device, dtype=torch.int32)
    check(_lib.load().segan_f0_eval(_ptr(f0_ref), _ptr(lag_ref), _ptr(f0_deg), _ptr(lag_deg),
                                    _ptr(nframes), rows, F, _ptr(out), _stream()), 'f0_eval')
    return out


_P = _lib.PYIN_DEFINES    # the integer macros of include/segan_pyin.h
PYIN_NTHETA = _P['SEGAN_PYIN_NTHETA']
PYIN_BINS = _P['SEGAN_PYIN_BINS']
PYIN_W = _P['SEGAN_PYIN_W']
PYIN_WS_CAP = 1 << 30    # bytes of workspace one call of segan_pyin may take


def _pyin_srate(srate):
    if isinstance(srate, bool) or srate not in PITCH_RATES:
        raise ValueError('pyin: srate must be one of {}, got {!r}'.format(PITCH_RATES, srate))


def pyin_tables(srate=16000):
    """segan_pyin_tables (host only) as a dict of numpy fp64 arrays, the bits the kernels read:
    'C' [101], the running sum of the thresholds' Beta(2, 18) weights; 'edge' [166], the bin edges
    as periods in samples at `srate`, descending; 'A' [2, 23], the transition weights (stay,
    switch) by band offset."""
    import numpy as np
    _pyin_srate(srate)
    C = np.zeros(PYIN_NTHETA + 1, np.float64)
    edge = np.zeros(PYIN_BINS + 1, np.float64)
    A = np.zeros((2, 2 * PYIN_W + 1), np.float64)
    check(_lib.load().segan_pyin_tables(srate, C.ctypes.data, edge.ctypes.data, A.ctypes.data),
          'pyin_tables')
    return {'C': C, 'edge': edge, 'A': A}


def pyin_dims(rows, T, srate=16000):
    """segan_pyin_dims (host only) as a dict: frames of a row of T samples, ws_doubles for `rows`
    rows."""
    dims = (ctypes.c_int64 * 2)()
    check(_lib.load().segan_pyin_dims(rows, T, srate, dims), 'pyin')
    return dict(zip(('frames', 'ws_doubles'), list(dims)))


def _pyin_run(x, lengths, srate, ws_cap, stages):
    _chk(x, 'x', 2)
    rows, T = x.shape
    if not 1 <= rows <= 65535 or not 1 <= T <= PITCH_MAX_T:
        raise ValueError('pyin: 1 .. 65535 rows of 1 .. 2^24 samples, got {}'.format(
            tuple(x.shape)))
    _pyin_srate(srate)
    lens = None if lengths is None else _row_lengths('pyin', lengths, rows, T, x.device)
    cap = _int_arg(ws_cap, 'pyin: ws_cap', 1, 1 << 62)
    lib = _lib.load()
    d = pyin_dims(1, T, srate)
    F = d['frames']
    per = int(cap // max(8 * d['ws_doubles'], 1))
    if per < 1:
        raise ValueError('pyin: ws_cap of {} bytes is below the {} bytes one row of {} samples '
                         'needs'.format(cap, 8 * d['ws_doubles'], T))
    per = min(per, rows)
    ws = _stream_scratch(max(8 * d['ws_doubles'] * per, 8), x.device)
    f64 = dict(device=x.device, dtype=torch.float64)
    i32 = dict(device=x.device, dtype=torch.int32)
    Fa = max(F, 1)
    f0 = torch.empty((rows, Fa), **f64)
    vp = torch.empty((rows, Fa), **f64)
    lag = torch.empty((rows, Fa), **i32)
    bv = torch.empty((rows, Fa, PYIN_BINS), **f64) if stages else None
    state = torch.empty((rows, Fa), **i32) if stages else None
    delta = torch.empty((rows, 2 * PYIN_BINS), **f64) if stages else None
    for r0 in range(0, rows, per):
        n = min(per, rows - r0)
        sl = slice(r0, r0 + n)
        check(lib.segan_pyin(_ptr(x[sl]), _ptr(None if lens is None else lens[sl]), n, T, srate,
                             _ptr(f0[sl]), _ptr(lag[sl]), _ptr(vp[sl]),
                             _ptr(bv[sl]) if stages else None,
                             _ptr(state[sl]) if stages else None,
                             _ptr(delta[sl]) if stages else None, _ptr(ws), _stream()), 'pyin')
    if lens is None:
        nframes = torch.full((rows,), F, **i32)
    else:
        host = lens.cpu().tolist()
        nframes = torch.tensor([lib.segan_pitch_frames(L, srate) for L in host],
                               dtype=torch.int32).to(x.device)
    out = {'f0': f0[:, :F], 'lag': lag[:, :F], 'vprob': vp[:, :F], 'nframes': nframes}
    if stages:
        out.update(bv=bv[:, :F], state=state[:, :F], delta=delta)
    return out


def pyin_stages(x, lengths=None, srate=16000, ws_cap=PYIN_WS_CAP):
    """`pyin` with its intermediates as a dict of device tensors: 'f0',
    'lag', 'vprob' [rows, F], 'nframes' [rows] (int32), 'bv' [rows, F, 165] (the voiced
    observation of every frame and bin, NaN from the row's own frame count on), 'state' [rows, F]
    (int32: the decoded state, bin m when voiced and 165 + m when unvoiced, -1 from the row's count
    on) and 'delta' [rows, 330] (the last frame's scaled Viterbi values, NaN for a row without a
    frame)."""
    return _pyin_run(x, lengths, srate, ws_cap, True)


def pyin(x, lengths=None, srate=16000, ws_cap=PYIN_WS_CAP):
    """The Viterbi-smoothed pitch contour of each row of x [rows, T] (fp32 CUDA tensor) at `srate`
    (16000 or 8000): pYIN (Mauch & Dixon 2014) on `pitch`'s framing, fp64 on the device: YIN
    candidates under 100 thresholds with a Beta(2, 18) prior, then a hidden Markov model over 165
    pitch bins (5 per semitone from 60 Hz) x {voiced, unvoiced} decoded by Viterbi.  Returns (f0
    [rows, F] in Hz, 0 when unvoiced; lag [rows, F] int32, the period picked in samples, 0 when
    unvoiced; vprob [rows, F], the frame's probability of being voiced before the decoding;
    nframes [rows] int32) under `pitch`'s contract, so `f0_eval` takes f0 and lag unchanged:
    frames from the row's own count on hold f0 = 0, lag = -1, vprob = NaN.  `lengths` and `ws_cap`
    as for `pitch`.  Fixed operation order: a batched row equals its own call bit for bit, and a
    row times a power of two gives the same bits."""
    out = _pyin_run(x, lengths, srate, ws_cap, False)
    return out['f0'], out['lag'], out['vprob'], out['nframes']


DENOISE_RULES ={'wiener': _D['SEGAN_DENOISE_WIENER'], 'logmmse': _D['SEGAN_DENOISE_LOGMMSE']}
DENOISE_RATES = (8000, 16000)
DENOISE_MAX_T = 1 << 24
DENOISE_WS_CAP = 1 << 30     # bytes of workspace one call of segan_denoise may take
_DENOISE_DT = {torch.float32: _D['SEGAN_DT_F32'], torch.float64: _D['SEGAN_DT_F64']}


def denoise_dims(rows, T, srate=16000):
    """segan_denoise_dims (host only) as a dict: frame, hop and nfft at `srate`, the frames of a
    row of T samples, ws_bytes for `rows` rows."""
    dims = (ctypes.c_int64 * 5)()
    check(_lib.load().segan_denoise_dims(rows, T, srate, dims), 'denoise')
    return dict(zip(('frame', 'hop', 'nfft', 'frames', 'ws_bytes'), list(dims)))


def _denoise_run(x, lengths, srate, rule, out_dtype, ws_cap, stages):
    if not isinstance(x, torch.Tensor):
        raise TypeError('x must be a tensor, got {}'.format(type(x)))
    if x.dtype not in _DENOISE_DT:
        raise TypeError('x must be float32 or float64, got {}'.format(x.dtype))
    _chk(x, 'x', None, x.dtype)
    if x.dim() not in (1, 2):
        raise ValueError('denoise: x must be [rows, T] or [T], got {}'.format(tuple(x.shape)))
    x2 = x.reshape(-1, x.shape[-1])
    rows, T = x2.shape
    if not 1 <= rows <= 65535 or not 1 <= T <= DENOISE_MAX_T:
        raise ValueError('denoise: 1 .. 65535 rows of 1 .. 2^24 samples, got {}'.format(
            tuple(x.shape)))
    if isinstance(srate, bool) or srate not in DENOISE_RATES:
        raise ValueError('denoise: srate must be one of {}, got {!r}'.format(DENOISE_RATES, srate))
    if not isinstance(rule, str) or rule not in DENOISE_RULES:
        raise ValueError('denoise: rule must be one of {}, got {!r}'.format(
            sorted(DENOISE_RULES), rule))
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DENOISE_DT:
        raise ValueError('denoise: out_dtype must be torch.float32 or torch.float64, got '
                         '{!r}'.format(out_dtype))
    lens = None if lengths is None else _row_lengths('denoise', lengths, rows, T, x.device)
    cap = _int_arg(ws_cap, 'denoise: ws_cap', 1, 1 << 62)
    lib = _lib.load()
    d = denoise_dims(1, T, srate)
    per = int(cap // d['ws_bytes'])
    if per < 1:
        raise ValueError('denoise: ws_cap of {} bytes is below the {} bytes one row of {} samples '
                         'needs'.format(cap, d['ws_bytes'], T))
    per = min(per, rows)
    ws = _stream_scratch(d['ws_bytes'] * per + 16, x.device)
    ws = ws[(-ws.data_ptr()) % 16:]
    nfmax = d['frames']
    y = torch.empty((rows, T), device=x.device, dtype=out_dtype)
    nframes = torch.empty(rows, device=x.device, dtype=torch.int32)
    vad = upd = None
    if stages:
        vad = torch.empty((rows, max(nfmax, 1)), device=x.device, dtype=torch.float64)
        upd = torch.empty((rows, max(nfmax, 1)), device=x.device, dtype=torch.int32)
    for r0 in range(0, rows, per):
        n = min(per, rows - r0)
        check(lib.segan_denoise(_ptr(x2[r0:r0 + n]), _DENOISE_DT[x.dtype],
                                _ptr(None if lens is None else lens[r0:r0 + n]), n, T, srate,
                                DENOISE_RULES[rule], _ptr(y[r0:r0 + n]), _DENOISE_DT[out_dtype],
                                _ptr(nframes[r0:r0 + n]),
                                _ptr(None if vad is None else vad[r0:r0 + n]),
                                _ptr(None if upd is None else upd[r0:r0 + n]), _ptr(ws),
                                _stream()), 'denoise')
    out = {'y': y.reshape(x.shape), 'nframes': nframes}
    if stages:
        out['vad'], out['noise_update'] = vad[:, :nfmax], upd[:, :nfmax]
    return out


def denoise_stages(x, lengths=None, srate=16000, rule='logmmse', out_dtype=None,
                   ws_cap=DENOISE_WS_CAP):
    """`denoise_rows` with what its decisions rest on, as a dict of device
    tensors: 'y' (shaped like x), 'nframes' [rows] (int32: each row's own frame count, 0 for a row
    returned unchanged), 'vad' [rows, nf of T] (fp64: v_t, the mean log likelihood ratio of the
    frame; NaN from the row's own count on) and 'noise_update' [rows, nf of T] (int32: 1 where
    v_t < 0.15 and the noise estimate took the frame in, else 0; -1 from the row's own count
    on)."""
    return _denoise_run(x, lengths, srate, rule, out_dtype, ws_cap, True)


def denoise_rows(x, lengths=None, srate=16000, rule='logmmse', out_dtype=None,
                 ws_cap=DENOISE_WS_CAP):
    """The Wiener (`rule='wiener'`, Scalart & Filho 1996) or log-MMSE (`rule='logmmse'`, Ephraim &
    Malah 1985) enhancement of each row of x ([rows, T] or [T], fp32 or fp64 CUDA tensor) at
    `srate` (16000 or 8000) on the device, all arithmetic fp64: 20 ms Hamming frames at half
    overlap, a 40 ms DFT, the decision-directed a-priori SNR (0.98), the noise spectrum taken
    from the first 120 ms and updated in the frames a likelihood-ratio VAD calls noise.  The
    definition is scripts/denoise_oracle.py.  Row r is x[r, :lengths[r]] (host integers 0 .. T;
    all T without `lengths`); a row shorter than 120 ms is returned unchanged; the output is zero
    from (nframes + 1) hops on, and of `out_dtype` (torch.float32, rounded once, or
    torch.float64; x's own by default).  The rows are processed in chunks whose workspace stays
    under `ws_cap` bytes.  Fixed operation order: a batched row equals its own call bit for bit,
    whatever the chunking."""
    return _denoise_run(x, lengths, srate, rule, out_dtype, ws_cap, False)['y']


_O = _lib.OMLSA_DEFINES  # the integer macros of include/segan_omlsa.h
OMLSA_U = _O['SEGAN_OMLSA_U']    # slots of the minimum window
OMLSA_V = _O['SEGAN_OMLSA_V']    # frames per slot
OMLSA_WS_CAP = 1 << 30       # bytes of workspace one call of segan_omlsa may take


def omlsa_dims(rows, T, srate=16000):
    """segan_omlsa_dims (host only) as a dict: frame, hop and nfft at `srate`, the frames of a row
    of T samples, ws_bytes for `rows` rows."""
    dims = (ctypes.c_int64 * 5)()
    check(_lib.load().segan_omlsa_dims(rows, T, srate, dims), 'omlsa')
    return dict(zip(('frame', 'hop', 'nfft', 'frames', 'ws_bytes'), list(dims)))


def _omlsa_run(x, lengths, srate, out_dtype, ws_cap, stages):
    if not isinstance(x, torch.Tensor):
        raise TypeError('x must be a tensor, got {}'.format(type(x)))
    if x.dtype not in _DENOISE_DT:
        raise TypeError('x must be float32 or float64, got {}'.format(x.dtype))
    _chk(x, 'x', None, x.dtype)
    if x.dim() not in (1, 2):
        raise ValueError('omlsa: x must be [rows, T] or [T], got {}'.format(tuple(x.shape)))
    x2 = x.reshape(-1, x.shape[-1])
    rows, T = x2.shape
    if not 1 <= rows <= 65535 or not 1 <= T <= DENOISE_MAX_T:
        raise ValueError('omlsa: 1 .. 65535 rows of 1 .. 2^24 samples, got {}'.format(
            tuple(x.shape)))
    if isinstance(srate, bool) or srate not in DENOISE_RATES:
        raise ValueError('omlsa: srate must be one of {}, got {!r}'.format(DENOISE_RATES, srate))
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DENOISE_DT:
        raise ValueError('omlsa: out_dtype must be torch.float32 or torch.float64, got '
                         '{!r}'.format(out_dtype))
    lens = None if lengths is None else _row_lengths('omlsa', lengths, rows, T, x.device)
    cap = _int_arg(ws_cap, 'omlsa: ws_cap', 1, 1 << 62)
    lib = _lib.load()
    d = omlsa_dims(1, T, srate)
    per = int(cap // d['ws_bytes'])
    if per < 1:
        raise ValueError('omlsa: ws_cap of {} bytes is below the {} bytes one row of {} samples '
                         'needs'.format(cap, d['ws_bytes'], T))
    per = min(per, rows)
    ws = _stream_scratch(d['ws_bytes'] * per + 16, x.device)
    ws = ws[(-ws.data_ptr()) % 16:]
    F, nfmax = d['frame'], d['frames']
    y = torch.empty((rows, T), device=x.device, dtype=out_dtype)
    nframes = torch.empty(rows, device=x.device, dtype=torch.int32)
    pres = rough = noise = None
    if stages:
        pres = torch.empty((rows, max(nfmax, 1)), device=x.device, dtype=torch.float64)
        rough = torch.empty((rows, max(nfmax, 1)), device=x.device, dtype=torch.int32)
        noise = torch.empty((rows, F + 1), device=x.device, dtype=torch.float64)
    for r0 in range(0, rows, per):
        n = min(per, rows - r0)
        check(lib.segan_omlsa(_ptr(x2[r0:r0 + n]), _DENOISE_DT[x.dtype],
                              _ptr(None if lens is None else lens[r0:r0 + n]), n, T, srate,
                              _ptr(y[r0:r0 + n]), _DENOISE_DT[out_dtype],
                              _ptr(nframes[r0:r0 + n]),
                              _ptr(None if pres is None else pres[r0:r0 + n]),
                              _ptr(None if rough is None else rough[r0:r0 + n]),
                              _ptr(None if noise is None else noise[r0:r0 + n]), _ptr(ws),
                              _stream()), 'omlsa')
    out = {'y': y.reshape(x.shape), 'nframes': nframes}
    if stages:
        out['presence'], out['rough'], out['noise'] = pres[:, :nfmax], rough[:, :nfmax], noise
    return out


def omlsa_stages(x, lengths=None, srate=16000, out_dtype=None, ws_cap=OMLSA_WS_CAP):
    """`omlsa_rows` with what its decisions rest on, as a dict of device
    tensors: 'y' (shaped like x), 'nframes' [rows] (int32: each row's own frame count, 0 for a row
    returned unchanged), 'presence' [rows, nf of T] (fp64: the weighted mean over the bins of the
    speech-presence probability p of the frame; NaN from the row's own count on), 'rough'
    [rows, nf of T] (int32: the bins that the rough decision of the first iteration called noise;
    -1 from the row's own count on) and 'noise' [rows, frame + 1] (fp64: the noise spectrum as the
    row's last frame used it; NaN for a row without frames)."""
    return _omlsa_run(x, lengths, srate, out_dtype, ws_cap, True)


def omlsa_rows(x, lengths=None, srate=16000, out_dtype=None, ws_cap=OMLSA_WS_CAP):
    """The OM-LSA enhancement (Cohen & Berdugo 2001) of each row of x ([rows, T] or [T], fp32 or
    fp64 CUDA tensor) at `srate` (16000 or 8000) on the device, all arithmetic fp64: the framing
    of `denoise_rows`, the log-spectral-amplitude gain weighted with the speech-presence
    probability, and the noise spectrum of IMCRA (Cohen 2003), which follows the minima of the
    smoothed periodogram over the last OMLSA_U * OMLSA_V frames and so needs no leading noise
    segment and keeps adapting when the level of the noise changes.  The definition is
    scripts/omlsa_oracle.py.  Row r is x[r, :lengths[r]] (host integers 0 .. T; all T without
    `lengths`); a row shorter than 120 ms is returned unchanged; the output is zero from
    (nframes + 1) hops on, and of `out_dtype` (torch.float32, rounded once, or torch.float64; x's
    own by default).  The rows are processed in chunks whose workspace stays under `ws_cap`
    bytes.  Fixed operation order: a batched row equals its own call bit for bit, whatever the
    chunking."""
    return _omlsa_run(x, lengths, srate, out_dtype, ws_cap, False)['y']


_R = _lib.RIR_DEFINES  # the integer macros of include/segan_rir.h
RIR_TILE = _R['SEGAN_RIR_TILE']      # samples per workgroup
RIR_GEOM = _R['SEGAN_RIR_GEOM']      # doubles per room: L, s, r, beta
RIR_MAX_T = _R['SEGAN_RIR_MAX_T']
RIR_RATES = (16000, 8000)
RIR_C = 343.0                        # m/s


def rir_dims(count, T, srate=16000):
    """segan_rir_dims (host only) as a dict: half_width (Hw = srate / 250), stride (entries per
    wall of the power tables), tiles of a row of T samples, ws_bytes for `count` responses."""
    dims = (ctypes.c_int64 * 4)()
    check(_lib.load().segan_rir_dims(count, T, srate, dims), 'rir')
    return dict(zip(('half_width', 'stride', 'tiles', 'ws_bytes'), list(dims)))


def rir_tables(beta, n_max):
    """The powers of the reflection coefficients, built on the host: beta [count, 6] or [6] ->
    numpy fp64 [count, 6, n_max + 1] with tab[.., 0] = 1 and tab[.., i] = tab[.., i - 1] * beta,
    one rounding per entry (0^0 = 1).  The oracle and the device read these bits."""
    import numpy as np
    beta = np.asarray(beta, np.float64).reshape(-1, 6)
    n_max = _int_arg(n_max, 'rir: n_max', 0, 1 << 24)
    tab = np.ones(beta.shape + (n_max + 1,), np.float64)
    for i in range(1, n_max + 1):
        tab[..., i] = tab[..., i - 1] * beta
    return tab


def _rir_geom(room, src, mic, beta):
    """room, src, mic [count, 3] or [3] and beta [count, 6] or [6] (a single row is repeated) as
    numpy fp64 [count, 15]; the library checks the values."""
    import numpy as np
    parts = []
    for name, v, w in (('room', room, 3), ('src', src, 3), ('mic', mic, 3), ('beta', beta, 6)):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        a = np.asarray(v, np.float64)
        if a.ndim not in (1, 2) or a.shape[-1] != w or a.size == 0:
            raise ValueError('rir: {} must be [count, {}] or [{}], got {}'.format(
                name, w, w, a.shape))
        parts.append(a.reshape(-1, w))
    count = max(len(a) for a in parts)
    for i, a in enumerate(parts):
        if len(a) not in (1, count):
            raise ValueError('rir: room, src, mic and beta must agree on count, got {}'.format(
                [len(p) for p in parts]))
        parts[i] = np.broadcast_to(a, (count, a.shape[1]))
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def _rir_run(room, src, mic, beta, taps, srate, lengths, stages):
    geom = _rir_geom(room, src, mic, beta)
    count = len(geom)
    T = _int_arg(taps, 'rir: taps', 1, RIR_MAX_T)
    if isinstance(srate, bool) or srate not in RIR_RATES:
        raise ValueError('rir: srate must be one of {}, got {!r}'.format(RIR_RATES, srate))
    if not 1 <= count <= 65535:
        raise ValueError('rir: 1 .. 65535 rooms, got {}'.format(count))
    if not torch.cuda.is_available():
        raise RuntimeError('rir: segan_pytorch_amd runs only on an MI355X (HIP) device; there is '
                           'no CPU path')
    device = torch.device('cuda', torch.cuda.current_device())
    lens = None if lengths is None else _row_lengths('rir', lengths, count, T, device)
    lib = _lib.load()
    d = rir_dims(count, T, srate)
    tables = torch.from_numpy(rir_tables(geom[:, 9:15], d['stride'] - 1)).to(device)
    ws = _stream_scratch(d['ws_bytes'] + 8, device)
    ws = ws[(-ws.data_ptr()) % 8:]
    h = torch.empty((count, T), device=device, dtype=torch.float64)
    images = torch.empty(count, device=device, dtype=torch.int64) if stages else None
    check(lib.segan_rir(geom.ctypes.data_as(ctypes.c_void_p), _ptr(tables), _ptr(lens), count, T,
                        srate, _ptr(h), _ptr(images), _ptr(ws), _stream()), 'rir')
    out = {'h': h}
    if stages:
        out['images'], out['geom'], out['tables'] = images, geom, tables
    return out


def rir_stages(room, src, mic, beta, taps, srate=16000, lengths=None):
    """`rir_shoebox` with what it rests on, as a dict: 'h' [count, taps] (fp64, device), 'images'
    [count] (int64, device: the images that reach each row, whatever their amplitude), 'geom'
    (numpy fp64 [count, 15]: L, s, r, beta as the library received them) and 'tables' (fp64 device
    [count, 6, stride]: `rir_tables`)."""
    return _rir_run(room, src, mic, beta, taps, srate, lengths, True)


def rir_shoebox(room, src, mic, beta, taps, srate=16000, lengths=None):
    """Room impulse responses of shoebox rooms by the image-source method (Allen & Berkley 1979,
    fractional delays by Peterson's Hann-windowed sinc of 8 ms) on the device, all arithmetic fp64;
    the definition is scripts/rir_oracle.py.  room [count, 3] (metres, 1 ..
    50 per axis), src and mic [count, 3] (strictly inside, at least 0.05 m apart), beta [count, 6]
    (reflection coefficients in 0 .. 1 of the walls x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz);
    host arrays, a single row is repeated.  Returns fp64 [count, taps] on the current device with
    the physical scale 1 / (4 pi d); row i is zero from lengths[i] on (host integers 0 .. taps).
    c = 343 m/s; no high-pass, no directivity, no air absorption.  Fixed operation order: a row's
    bits depend neither on the other rows, nor on taps, nor on lengths beyond the masking."""
    return _rir_run(room, src, mic, beta, taps, srate, lengths, False)['h']


_E = _lib.EXT_DEFINES   # the integer macros of include/segan_dereverb.h
WPE_RATES = (8000, 16000)
WPE_MAX_T = 1 << 24
WPE_MAX_TAPS = _E['SEGAN_WPE_MAX_TAPS']
WPE_MAX_DELAY = _E['SEGAN_WPE_MAX_DELAY']
WPE_MAX_ITERATIONS = _E['SEGAN_WPE_MAX_ITERATIONS']
WPE_TILE = _E['SEGAN_WPE_TILE']            # frames the hot kernel streams a long row with
WPE_PIVOT = _E['SEGAN_WPE_ST_PIVOT']       # status bit of wpe_rows
WPE_WS_CAP = 1 << 30         # bytes of workspace one call of segan_wpe may take


def wpe_dims(rows, T, srate=16000, taps=10, delay=3):
    """segan_wpe_dims (host only) as a dict: nfft, hop and bins at `srate`, the frames of a row of
    T samples, ws_bytes for `rows` rows."""
    dims = (ctypes.c_int64 * 5)()
    check(_lib.load().segan_wpe_dims(rows, T, srate, taps, delay, dims), 'wpe')
    return dict(zip(('nfft', 'hop', 'bins', 'frames', 'ws_bytes'), list(dims)))


def _wpe_run(x, lengths, srate, taps, delay, iterations, out_dtype, ws_cap, stages):
    if not isinstance(x, torch.Tensor):
        raise TypeError('x must be a tensor, got {}'.format(type(x)))
    if x.dtype not in _DENOISE_DT:
        raise TypeError('x must be float32 or float64, got {}'.format(x.dtype))
    _chk(x, 'x', None, x.dtype)
    if x.dim() not in (1, 2):
        raise ValueError('wpe: x must be [rows, T] or [T], got {}'.format(tuple(x.shape)))
    x2 = x.reshape(-1, x.shape[-1])
    rows, T = x2.shape
    if not 1 <= rows <= 65535 or not 1 <= T <= WPE_MAX_T:
        raise ValueError('wpe: 1 .. 65535 rows of 1 .. 2^24 samples, got {}'.format(tuple(x.shape)))
    if isinstance(srate, bool) or srate not in WPE_RATES:
        raise ValueError('wpe: srate must be one of {}, got {!r}'.format(WPE_RATES, srate))
    taps = _int_arg(taps, 'wpe: taps', 1, WPE_MAX_TAPS)
    delay = _int_arg(delay, 'wpe: delay', 1, WPE_MAX_DELAY)
    iterations = _int_arg(iterations, 'wpe: iterations', 0, WPE_MAX_ITERATIONS)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DENOISE_DT:
        raise ValueError('wpe: out_dtype must be torch.float32 or torch.float64, got '
                         '{!r}'.format(out_dtype))
    lens = None if lengths is None else _row_lengths('wpe', lengths, rows, T, x.device)
    cap = _int_arg(ws_cap, 'wpe: ws_cap', 1, 1 << 62)
    lib = _lib.load()
    d = wpe_dims(1, T, srate, taps, delay)
    per = int(cap // d['ws_bytes'])
    if per < 1:
        raise ValueError('wpe: ws_cap of {} bytes is below the {} bytes one row of {} samples '
                         'needs'.format(cap, d['ws_bytes'], T))
    per = min(per, rows)
    ws = _stream_scratch(d['ws_bytes'] * per + 16, x.device)
    ws = ws[(-ws.data_ptr()) % 16:]
    F, nfmax = d['bins'], d['frames']
    y = torch.empty((rows, T), device=x.device, dtype=out_dtype)
    nframes = torch.empty(rows, device=x.device, dtype=torch.int32)
    status = torch.empty(rows, device=x.device, dtype=torch.int32)
    Y = X = g = None
    if stages:
        Y = torch.empty((rows, F, nfmax), device=x.device, dtype=torch.complex128)
        X = torch.empty((rows, F, nfmax), device=x.device, dtype=torch.complex128)
        g = torch.empty((rows, F, taps), device=x.device, dtype=torch.complex128)
    for r0 in range(0, rows, per):
        n = min(per, rows - r0)
        check(lib.segan_wpe(_ptr(x2[r0:r0 + n]), _DENOISE_DT[x.dtype],
                            _ptr(None if lens is None else lens[r0:r0 + n]), n, T, srate, taps,
                            delay, iterations, _ptr(y[r0:r0 + n]), _DENOISE_DT[out_dtype],
                            _ptr(nframes[r0:r0 + n]), _ptr(status[r0:r0 + n]),
                            _ptr(None if Y is None else Y[r0:r0 + n]),
                            _ptr(None if X is None else X[r0:r0 + n]),
                            _ptr(None if g is None else g[r0:r0 + n]), _ptr(ws), _stream()),
              'wpe')
    out = {'y': y.reshape(x.shape), 'nframes': nframes, 'status': status}
    if stages:
        out['Y'], out['X'], out['g'] = Y, X, g
    return out


def wpe_stages(x, lengths=None, srate=16000, taps=10, delay=3, iterations=3, out_dtype=None,
               ws_cap=WPE_WS_CAP):
    """`wpe_rows` with its stages, as a dict of device tensors: 'y' (shaped
    like x), 'nframes' [rows] (int32: each row's own frame count), 'status' [rows] (int32: 0, or
    WPE_PIVOT where a bin's Cholesky met a pivot that is not positive and the bin was left
    unfiltered), 'Y' and 'X' [rows, bins, nf of T] (complex128: the STFT and the filtered STFT,
    bin-major, zero from the row's own count on) and 'g' [rows, bins, taps] (complex128: the last
    prediction filter of every bin; zero for a row returned unchanged)."""
    return _wpe_run(x, lengths, srate, taps, delay, iterations, out_dtype, ws_cap, True)


def wpe_rows(x, lengths=None, srate=16000, taps=10, delay=3, iterations=3, out_dtype=None,
             ws_cap=WPE_WS_CAP):
    """The WPE dereverberation (weighted prediction error, Nakatani et al. 2010, single channel)
    of each row of x ([rows, T] or [T], fp32 or fp64 CUDA tensor) at `srate` (16000 or 8000) on
    the device, all arithmetic fp64: a 32 ms square-root Hann STFT at a quarter hop, and per bin
    `iterations` (0 .. 8) rounds of a `taps`-frame (1 .. 32) linear prediction from the frames
    `delay` (1 .. 8) and more back, weighted by the inverse power of the current estimate, whose
    prediction is subtracted.  The definition is scripts/wpe_oracle.py.  Row r is
    x[r, :lengths[r]] (host integers 0 .. T; all T without `lengths`); a row of at most delay +
    taps frames is returned unchanged; the output is zero from the row's length on, and of
    `out_dtype` (torch.float32, rounded once, or torch.float64; x's own by default).  The rows are
    processed in chunks whose workspace stays under `ws_cap` bytes.  Fixed operation order: a
    batched row equals its own call bit for bit, whatever the chunking."""
    return _wpe_run(x, lengths, srate, taps, delay, iterations, out_dtype, ws_cap, False)['y']


ASL_THRESHOLDS = 15      # nbits - 1 thresholds 2^-15 .. 2^-1 (nbits = 16)
ADDITIVE_CAP = 1         # status bits of asl_p56 / additive_mix (include/segan_hip.h)
ADDITIVE_PN0 = 2
ADDITIVE_RANGE = 4


def asl_p56_stages(x, srate=16000, nbits=16, lengths=None, _want_q=True):
    """ITU-T P.56 method-B active speech level of each row of x [rows, T] (fp32 CUDA tensor), the
    reference's `Additive.asl_P56` (utils.py:180-297) in fp64 on the device.
    Row r is x[r, :lengths[r]] (all T without `lengths`; host integers as in `stoi_stages`).
    Returns a dict of device tensors: sq [rows] (sum of squares), asl_ms (active-level mean
    square), asl (activity factor), c0 (threshold; NaN where the reference returns None, and then
    asl_ms = asl = 0), counts int32 [rows, 15] (activity counts per threshold 2^-15 .. 2^-1),
    status int32 [rows] (1: the interpolation's iteration cap was reached) and q fp64 [rows, T]
    (the envelope, zero past the row's length).  nbits must be 16."""
    _chk(x, 'x', 2)
    srate = _int_arg(srate, 'asl_p56: srate', 1, 768000)
    if _int_arg(nbits, 'asl_p56: nbits', 2, 64) != ASL_THRESHOLDS + 1:
        raise NotImplementedError('asl_p56: nbits={} is not supported (16 only)'.format(nbits))
    rows, T = x.shape
    if rows == 0 or T == 0:
        raise ValueError('asl_p56: empty input {}'.format(tuple(x.shape)))
    lens = None if lengths is None else _row_lengths('asl_p56', lengths, rows, T, x.device)
    level = torch.empty((rows, 4), device=x.device, dtype=torch.float64)
    counts = torch.empty((rows, ASL_THRESHOLDS), device=x.device, dtype=torch.int32)
    status = torch.empty(rows, device=x.device, dtype=torch.int32)
    q = torch.empty((rows, T), device=x.device, dtype=torch.float64) if _want_q else None
    check(_lib.load().segan_asl_p56(_ptr(x), _ptr(lens), rows, T, srate, ASL_THRESHOLDS + 1,
                                    _ptr(level), _ptr(counts), _ptr(status), _ptr(q), _stream()),
          'asl_p56')
    out = dict(sq=level[:, 0], asl_ms=level[:, 1], asl=level[:, 2], c0=level[:, 3], counts=counts,
               status=status)
    if _want_q:
        out['q'] = q
    return out


def asl_p56(x, srate=16000, nbits=16, lengths=None):
    """`asl_p56_stages` without the envelope: dict(sq, asl_ms, asl, c0, counts, status) of device
    tensors.  No device-to-host copy."""
    return asl_p56_stages(x, srate, nbits, lengths, _want_q=False)


def _upload(t, device):
    """The host tensor t on `device`, through pinned staging in an asynchronous copy: a pageable
    copy would hold the host until everything queued on this stream before it (the loader's 20 MB
    batch copy) has finished.  Pinned only when the target is a HIP device."""
    if torch.device(device).type == 'cuda':
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def _host_rows(what, name, v, shape, dtype, check_host=None):
    """Per-row host values as a contiguous CPU tensor of `dtype` and `shape`; `check_host` sees
    them in their own dtype first."""
    # through numpy: python floats stay float64 (torch.as_tensor would make them float32)
    t = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    n = 1
    for s in shape:
        n *= s
    if t.numel() != n or t.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError('{}: {} must hold {} values, got {}'.format(
            what, name, ' x '.join(str(s) for s in shape), list(t.shape)))
    if not dtype.is_floating_point and t.dtype.is_floating_point:
        raise ValueError('{}: {} must be integers'.format(what, name))
    t = t.reshape(shape)
    if check_host is not None:
        check_host(t)
    return t.to(dtype).contiguous()


def _row_arg(what, name, v, shape, dtype, device, check_host=None):
    """A per-row argument on `device`: a CUDA tensor of `dtype` and `shape` is used as it is (its
    values are the caller's business: the kernels flag what they cannot use); host values are
    checked by `check_host` and uploaded (`_host_rows`, `_upload`)."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype != dtype or tuple(v.shape) != tuple(shape) or v.device != device:
            raise ValueError('{}: device {} must be {} {} on {}, got {} {}'.format(
                what, name, dtype, list(shape), device, v.dtype, list(v.shape)))
        return v.contiguous()
    return _upload(_host_rows(what, name, v, shape, dtype, check_host), device)


def _fits_int32(what, name, t):
    if int(t.min()) < -(1 << 31) or int(t.max()) >= 1 << 31:
        raise ValueError('{}: {} do not fit 32 bits'.format(what, name))


def _level_arg(what, name, t, rows):
    """asl_ms or c0 of `asl_p56`: an fp64 CUDA tensor of one value per row.  They are columns of
    one block there, so a strided one is taken and made contiguous (which `_chk` would refuse)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and
            t.numel() == rows):
        raise TypeError('{}: {} must be a CUDA float64 tensor of {} values'.format(what, name, rows))
    return t.contiguous()


def _prev_arg(what, prev, rows, device):
    """prev (the sample preceding each row), when given: fp32 [rows] on `device`."""
    if prev is not None:
        _chk(prev, 'prev', 1)
        if prev.numel() != rows or prev.device != device:
            raise ValueError('{}: prev must hold {} values on {}'.format(what, rows, device))


def additive_mix(clean, bank, starts, snrs, px, lengths=None, prev=None):
    """clean [rows, T] + noise at a target SNR, the reference's `addnoise_asl` and anti-clipping
    loop (utils.py:98-134, 89-95) in fp64 on the device, rounded to fp32 once.  bank: the flat
    fp32 CUDA noise bank; starts (host integers [rows]): absolute index of each row's segment,
    checked here to lie inside the bank; snrs (host numbers [rows]): dB; px: fp64 CUDA tensor
    [rows], the rows' asl_ms from `asl_p56`.  prev (optional fp32 CUDA [rows]): the clean sample
    preceding each row; it is mixed with bank[start - 1] (start >= 1) and returned as
    info['prev'].  Returns (noisy [rows, T], info) with info = dict(Pn, sf fp64 [rows], n,
    status int32 [rows]): noise mean square, scale factor, number of anti-clipping divisions;
    status: ADDITIVE_CAP (the division cap was reached) | ADDITIVE_PN0 (a segment of digital
    silence: sf = 0, noisy == clean).  px == 0 gives sf = 0 and noisy == clean."""
    _chk(clean, 'clean', 2)
    _chk(bank, 'bank', 1)
    rows, T = clean.shape
    if rows == 0 or T == 0 or bank.numel() == 0:
        raise ValueError('additive_mix: empty input')
    px = _level_arg('additive_mix', 'px', px, rows)
    if bank.device != clean.device or px.device != clean.device:
        raise ValueError('additive_mix: tensors on different devices')
    # torch.as_tensor: snrs given as python floats are float32 values, as they have always been
    st = _host_rows('additive_mix', 'starts', torch.as_tensor(starts), (rows,), torch.int64)
    sn = _host_rows('additive_mix', 'snrs', torch.as_tensor(snrs), (rows,), torch.float64)
    lens = None if lengths is None else _row_lengths('additive_mix', lengths, rows, T, clean.device)
    need = torch.full((rows,), T, dtype=torch.int64) if lens is None else lens.cpu().to(torch.int64)
    lo = 1 if prev is not None else 0
    if int(st.min()) < lo or bool((st + need > bank.numel()).any()):
        raise ValueError('additive_mix: segment outside the noise bank of {} samples (starts {}, '
                         'lengths {})'.format(bank.numel(), st.tolist(), need.tolist()))
    if not bool(torch.isfinite(sn).all()):
        raise ValueError('additive_mix: snrs must be finite, got {}'.format(sn.tolist()))
    _prev_arg('additive_mix', prev, rows, clean.device)
    # one pinned staging buffer, one asynchronous copy: a pageable copy would hold the host until
    # everything queued on this stream before it (the loader's 20 MB batch copy) has finished
    args = torch.empty(2 * rows, dtype=torch.int64).pin_memory()
    args[:rows] = st
    args[rows:].view(torch.float64).copy_(sn)
    args = args.to(clean.device, non_blocking=True)
    st_d, sn_d = args[:rows], args[rows:].view(torch.float64)
    noisy = torch.empty_like(clean)
    prev_out = torch.empty_like(prev) if prev is not None else None
    info = torch.empty((rows, 2), device=clean.device, dtype=torch.float64)
    istat = torch.empty((rows, 2), device=clean.device, dtype=torch.int32)
    check(_lib.load().segan_additive_mix(_ptr(clean), _ptr(lens), _ptr(bank), bank.numel(),
                                         _ptr(st_d), _ptr(sn_d), _ptr(px), _ptr(prev),
                                         rows, T, _ptr(noisy), _ptr(prev_out), _ptr(info),
                                         _ptr(istat), _stream()), 'additive_mix')
    out = dict(Pn=info[:, 0], sf=info[:, 1], n=istat[:, 0], status=istat[:, 1])
    if prev is not None:
        out['prev'] = prev_out
    return noisy, out


RESAMPLE_RATES = (4000, 192000)
RESAMPLE_ZEROS = 32          # the one default of every layer: flat to 7.5 kHz and at most -89 dB
RESAMPLE_BETA = 8.6          # beyond 9 kHz for 48 -> 16 kHz.  (10, 5.0) is scipy's default.
RESAMPLE_ZEROS_MAX = 64
RESAMPLE_BETA_MAX = 20.0
_RESAMPLE_DT = {torch.float32: _D['SEGAN_DT_F32'], torch.int16: _D['SEGAN_DT_I16'], torch.float64: _D['SEGAN_DT_F64']}


def _resample_args(rate_in, rate_out, zeros, beta):
    rate_in = _int_arg(rate_in, 'resample: rate_in', *RESAMPLE_RATES)
    rate_out = _int_arg(rate_out, 'resample: rate_out', *RESAMPLE_RATES)
    zeros = _int_arg(zeros, 'resample: zeros', 1, RESAMPLE_ZEROS_MAX)
    try:
        b = None if isinstance(beta, bool) else float(beta)
    except (TypeError, ValueError):
        b = None
    if b is None or not 0.0 <= b <= RESAMPLE_BETA_MAX:
        raise ValueError('resample: beta must be a number from 0 to {}, got {!r}'.format(
            RESAMPLE_BETA_MAX, beta))
    return rate_in, rate_out, zeros, b


def resample_plan(rate_in, rate_out, zeros=RESAMPLE_ZEROS, beta=RESAMPLE_BETA):
    """The host-side plan of a conversion rate_in -> rate_out (no device involved): (p, q, taps)
    with p / q = rate_out / rate_in in lowest terms and the fp64 CPU tensor of 2 zeros max(p, q) + 1
    taps p h / sum(h), h[t] = sinc(t / max(p, q)) kaiser(beta) — scipy.signal.resample_poly's
    filter; (zeros, beta) = (10, 5.0) is scipy's default.  Equal rates: (1, 1, [1.0])."""
    rate_in, rate_out, zeros, beta = _resample_args(rate_in, rate_out, zeros, beta)
    lib = _lib.load()
    return _fetch_taps(lambda *a: lib.segan_resample_plan(rate_in, rate_out, zeros, beta, *a),
                       'resample_plan')


def resample_dims(T, rate_in, rate_out):
    """(Ly, tile): the samples T samples at rate_in become at rate_out, ceil(T p / q), and the
    number of consecutive outputs one workgroup of the kernel computes (host only)."""
    rate_in, rate_out, _, _ = _resample_args(rate_in, rate_out, 1, 0.0)
    dims = (ctypes.c_int * 2)()
    check(_lib.load().segan_resample_dims(_int_arg(T, 'resample: T', 0, 2 ** 31 - 1), rate_in,
                                          rate_out, dims), 'resample_dims')
    return dims[0], dims[1]


def resample(x, rate_in, rate_out, lengths=None, out_dtype=None, zeros=RESAMPLE_ZEROS,
             beta=RESAMPLE_BETA):
    """Sample-rate conversion of each row of x [rows, T] (a CUDA tensor, float32 or int16 with the
    values used as they are) from rate_in to rate_out Hz on the device, fp64 arithmetic (DESIGN.md
    section 12): scipy.signal.resample_poly's polyphase filter with a Kaiser window of `zeros`
    zero crossings a side and `beta` ((10, 5.0) is scipy's default).  Row r is x[r, :lengths[r]]
    (all T without `lengths`: host integers, or an int32 CUDA tensor that is used as it is and
    clamped to 0 .. T on the device).  out_dtype: torch.float64, torch.float32 (rounded once from
    the fp64 sum) or torch.int16 (rounded half to even, saturated); default: x's dtype.
    Returns (y [rows, ceil(T p / q)], info): row r holds info['lengths'][r] = ceil(len_r p / q)
    samples and zeros after them; info['nclip'][r] = its saturated samples (int16 output; 0
    otherwise).  Both are int32 device tensors.  No device-to-host copy."""
    if not isinstance(x, torch.Tensor):
        raise TypeError('resample: x must be a tensor, got {}'.format(type(x)))
    if not x.is_cuda:
        raise RuntimeError('resample: x is on {}: segan_pytorch_amd runs only on an MI355X (HIP) '
                           'device; there is no CPU path'.format(x.device))
    if x.dtype not in (torch.float32, torch.int16):
        raise TypeError('resample: x must be float32 or int16, got {}'.format(x.dtype))
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in _RESAMPLE_DT:
        raise TypeError('resample: out_dtype must be torch.float64, float32 or int16, got '
                        '{}'.format(out_dtype))
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError('resample: x must be [rows, T] and not empty, got {}'.format(tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError('resample: x must be contiguous')
    rate_in, rate_out, zeros, beta = _resample_args(rate_in, rate_out, zeros, beta)
    rows, T = x.shape
    lens = None if lengths is None else _row_lengths('resample', lengths, rows, T, x.device, True)
    lib = _lib.load()
    dims = (ctypes.c_int * 2)()
    check(lib.segan_resample_dims(T, rate_in, rate_out, dims), 'resample')
    Ly, tile = dims[0], dims[1]
    y = torch.empty((rows, Ly), device=x.device, dtype=out_dtype)
    out_lens = torch.empty(rows, device=x.device, dtype=torch.int32)
    nclip = torch.empty(rows, device=x.device, dtype=torch.int32)
    ws = None
    if out_dtype == torch.int16:
        ws = torch.empty(rows * ((Ly + tile - 1) // tile), device=x.device, dtype=torch.int32)
    check(lib.segan_resample(_ptr(x), _RESAMPLE_DT[x.dtype], _ptr(lens), rows, T, rate_in, rate_out,
                             zeros, beta, _ptr(y), _RESAMPLE_DT[out_dtype], Ly, _ptr(out_lens),
                             _ptr(nclip), _ptr(ws), _stream()), 'resample')
    return y, dict(lengths=out_lens, nclip=nclip)


def _index_arg(index, B, device, what):
    if index is None:
        return None, B
    idx = torch.as_tensor(index).detach().cpu().reshape(-1)
    if idx.dtype.is_floating_point or idx.dtype == torch.bool or idx.numel() == 0:
        raise ValueError('{}: index must hold integers, got {}'.format(what, index))
    if int(idx.min()) < 0 or int(idx.max()) >= B:
        raise ValueError('{}: index outside 0 .. {}: {}'.format(what, B - 1, idx.tolist()))
    return _upload(idx.to(torch.int32), device), idx.numel()


def pcm16_wave(pcm, index=None):
    """The clean rows of the int16 slices pcm [B, 2, T+1] (the layout of `pcm16_prep`) for the
    batch items `index` (host integers; None: all) as the fp32 min-max-normalised wave [n, T]
    (se_dataset.py:108-117, no pre-emphasis) and prev [n], the same of the sample preceding each
    slice."""
    if not isinstance(pcm, torch.Tensor) or pcm.dtype != torch.int16 or not pcm.is_cuda:
        raise TypeError('pcm16_wave: pcm must be a CUDA int16 tensor')
    if pcm.dim() != 3 or pcm.shape[1] != 2 or not pcm.is_contiguous() or pcm.shape[2] < 2:
        raise ValueError('pcm16_wave: pcm must be contiguous [B, 2, T+1]')
    B, T = pcm.shape[0], pcm.shape[2] - 1
    idx, n = _index_arg(index, B, pcm.device, 'pcm16_wave')
    if n == 0 or n > 65535:
        raise ValueError('pcm16_wave: 1 .. 65535 rows, got {}'.format(n))
    wave = torch.empty((n, T), device=pcm.device, dtype=torch.float32)
    prev = torch.empty(n, device=pcm.device, dtype=torch.float32)
    check(_lib.load().segan_pcm16_wave(ctypes.c_void_p(pcm.data_ptr()), _ptr(idx), _ptr(wave),
                                       _ptr(prev), n, B, T, _stream()), 'pcm16_wave')
    return wave, prev


def preemph_rows(x, prev, first, out, coef, index=None):
    """out[index[k]] = pre-emphasis of x[k] (fp32 CUDA [n, T]; out [B, T]): y[t] = x[t] - coef *
    x[t-1] in double, rounded once, with x[-1] = prev[k]; y[0] = x[0] where first[index[k]] (uint8
    CUDA [B]) is set.  Only the indexed rows of `out` are written; returns out."""
    _chk(x, 'x', 2)
    _chk(prev, 'prev', 1)
    _chk(out, 'out', 2)
    if not isinstance(first, torch.Tensor) or first.dtype != torch.uint8 or not first.is_cuda:
        raise TypeError('preemph_rows: first must be a CUDA uint8 tensor')
    B, T = out.shape
    n = x.shape[0]
    idx, ni = _index_arg(index, B, x.device, 'preemph_rows')
    if x.shape[1] != T or prev.numel() != n or first.numel() != B or ni != n or n == 0 or n > 65535:
        raise ValueError('preemph_rows: x [n, T], prev [n], first [B], out [B, T], index [n] '
                         '(n = B without index) expected')
    check(_lib.load().segan_preemph_rows(_ptr(x), _ptr(prev), ctypes.c_void_p(first.data_ptr()),
                                         _ptr(idx), _ptr(out), n, B, T, float(coef), _stream()),
          'preemph_rows')
    return out


# ---------------------------------------------------------------------------------
# reverberation
# ---------------------------------------------------------------------------------
REVERB_P = _D['SEGAN_REVERB_P']              # the partition; transforms are 2P
REVERB_RIR = _D['SEGAN_REVERB_ST_RIR']       # status bits of reverb_rows
REVERB_DELAY = _D['SEGAN_REVERB_ST_DELAY']
_reverb_bases = {}
_reverb_ws = {}


def reverb_dims(rows, T, max_delay, max_taps=None):
    """dict(P, blocks, frames, partitions, staging, spectrum, time, workspace) of
    `segan_reverb_dims`: blocks of P samples per row, rows of the two transforms' products, and
    the buffer sizes in floats."""
    dims = (ctypes.c_int64 * 8)()
    max_delay = _int_arg(max_delay, 'reverb_dims: max_delay', 0, 1 << 30)
    taps = max_delay + 1 if max_taps is None else _int_arg(max_taps, 'reverb_dims: max_taps', 1, 1 << 30)
    check(_lib.load().segan_reverb_dims(rows, T, max_delay, taps, dims), 'reverb_dims')
    return dict(zip(('P', 'blocks', 'frames', 'partitions', 'staging', 'spectrum', 'time',
                     'workspace'), (int(v) for v in dims)))


def reverb_basis(device):
    """(fwd [2P, 2P], inv [2P, P]): the shared DFT bases of the partitioned convolution, built once
    per device."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('reverb: segan_pytorch_amd runs only on an MI355X (HIP) device; there '
                           'is no CPU path')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device not in _reverb_bases:
        with torch.cuda.device(device):
            fwd = torch.empty((2 * REVERB_P, 2 * REVERB_P), device=device, dtype=torch.float32)
            inv = torch.empty((2 * REVERB_P, REVERB_P), device=device, dtype=torch.float32)
            check(_lib.load().segan_reverb_basis(_ptr(fwd), _ptr(inv), _stream()), 'reverb_basis')
            torch.cuda.current_stream(device).synchronize()   # other streams may use it next
        _reverb_bases[device] = (fwd, inv)
    return _reverb_bases[device]


def reverb_bank(taps):
    """taps [n_parts, P] (fp32 CUDA: the RIRs zero-padded to whole partitions) -> H [n_parts, 2P],
    the packed spectra of the partitions zero-padded to 2P."""
    _chk(taps, 'taps', 2)
    if taps.shape[1] != REVERB_P or taps.shape[0] == 0:
        raise ValueError('reverb_bank: taps must be [n_parts, {}], got {}'.format(
            REVERB_P, tuple(taps.shape)))
    fwd, _ = reverb_basis(taps.device)
    H = torch.empty((taps.shape[0], 2 * REVERB_P), device=taps.device, dtype=torch.float32)
    check(_lib.load().segan_reverb_bank(_ptr(taps), taps.shape[0], _ptr(fwd), _ptr(H), _stream()),
          'reverb_bank')
    return H


class ReverbBankData(object):
    """What `reverb_rows` needs of a bank on one device: H [n_parts, 2P] (`reverb_bank`), table
    int32 [n_rirs, 4] = (first partition, partitions, taps, delay) on the device, and the largest
    delay (a host integer: it sizes the buffers)."""

    def __init__(self, H, table, max_delay):
        _chk(H, 'H', 2)
        _chk(table, 'table', None, torch.int32)
        if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] == 0 or table.device != H.device:
            raise TypeError("ReverbBankData: table must be int32 [n_rirs, 4] on H's device")
        if H.shape[1] != 2 * REVERB_P or H.shape[0] == 0:
            raise ValueError('ReverbBankData: H must be [n_parts, {}]'.format(2 * REVERB_P))
        self.H, self.table = H, table
        self.max_delay = _int_arg(max_delay, 'ReverbBankData: max_delay', 0, 1 << 30)


def _reverb_args(x, bank, rir_ids, lengths, prev):
    _chk(x, 'x', 2)
    rows, T = x.shape
    if rows == 0 or T == 0:
        raise ValueError('reverb_rows: empty input {}'.format(tuple(x.shape)))
    if not isinstance(bank, (ReverbBankData, torch.Tensor)) and callable(getattr(bank, 'data', None)):
        bank = bank.data(x.device)      # an augment.RIRBank
    if not isinstance(bank, ReverbBankData):
        raise TypeError('reverb_rows: bank must be an augment.RIRBank or a ReverbBankData')
    if bank.H.device != x.device:
        raise ValueError('reverb_rows: tensors on different devices')
    ids = _row_arg('reverb_rows', 'rir_ids', rir_ids, (rows,), torch.int32, x.device,
                   lambda t: _fits_int32('reverb_rows', 'rir_ids', t))
    lens = None if lengths is None else _row_lengths('reverb_rows', lengths, rows, T, x.device)
    _prev_arg('reverb_rows', prev, rows, x.device)
    return bank, ids, lens


def _reverb_workspace(floats, device):
    """The chain's workspace (120 MB at [300, 16384]), kept per (device, stream) and grown on
    demand: calls on one stream run in order, so they can share it; another stream gets its own.
    The buffer is held for the life of the process (it only grows and is never released; an entry
    outlives its stream) — one per stream that ever reverberated, the loader's side stream in
    training."""
    key = (device, _stream().value)
    ws = _reverb_ws.get(key)
    if ws is None or ws.numel() < floats:
        ws = _reverb_ws[key] = torch.empty(floats, device=device, dtype=torch.float32)
    return ws


def reverb_rows(x, bank, rir_ids, lengths=None, prev=None):
    """x [rows, T] (fp32 CUDA) convolved row by row with the room impulse responses `rir_ids`
    (host integers or a CUDA int32 tensor, [rows]) of `bank` (an `augment.RIRBank`, or its
    `data(device)`): y[n] = sum_k h[k] x[n + d - k] with d the RIR's direct path (DESIGN.md section
    14), x[-1] = prev (optional fp32 CUDA [rows]), zero outside the row's `lengths`.  Returns
    (y [rows, T], info): info['prev'] = y[-1] (fp32 [rows]; what a pre-emphasis that follows
    needs), info['status'] int32 [rows]: REVERB_RIR (the id is not in the bank) | REVERB_DELAY;
    a flagged row is returned unchanged.  No device-to-host copy."""
    bank, ids, lens = _reverb_args(x, bank, rir_ids, lengths, prev)
    rows, T = x.shape
    fwd, inv = reverb_basis(x.device)
    dims = reverb_dims(rows, T, bank.max_delay)
    ws = _reverb_workspace(dims['workspace'], x.device)
    y = torch.empty_like(x)
    prev_out = torch.empty(rows, device=x.device, dtype=torch.float32)
    status = torch.empty(rows, device=x.device, dtype=torch.int32)
    check(_lib.load().segan_reverb_rows(
        _ptr(x), _ptr(lens), _ptr(prev), _ptr(bank.H), bank.H.shape[0], _ptr(ids),
        _ptr(bank.table), bank.table.shape[0], _ptr(fwd), _ptr(inv), rows, T, bank.max_delay,
        _ptr(ws), ws.numel(), _ptr(y), _ptr(prev_out), _ptr(status), _stream()), 'reverb_rows')
    return y, dict(prev=prev_out, status=status)


def reverb_stages(x, bank, rir_ids, lengths=None, prev=None, X=None, yt=None):
    """`reverb_rows` stage by stage through the library's separate entry points (tests, timing):
    returns dict(xs, X, Y, yt, y, prev, status, dims).  X / yt given: the delay line / the output
    stage run on those instead of on the products of the stages before."""
    bank, ids, lens = _reverb_args(x, bank, rir_ids, lengths, prev)
    rows, T = x.shape
    lib = _lib.load()
    fwd, inv = reverb_basis(x.device)
    dims = reverb_dims(rows, T, bank.max_delay)
    NB, M, P = dims['blocks'], dims['frames'], REVERB_P
    dev = x.device
    xs = torch.empty(dims['staging'], device=dev, dtype=torch.float32)
    check(lib.segan_reverb_stage(_ptr(x), _ptr(lens), _ptr(prev), _ptr(xs), rows, T, NB, M,
                                 _stream()), 'reverb_stage')
    if X is None:
        X = torch.empty((M, 2 * P), device=dev, dtype=torch.float32)
        check(lib.segan_reverb_forward(_ptr(xs), _ptr(fwd), _ptr(X), M, _stream()),
              'reverb_forward')
    Y = torch.empty((M, 2 * P), device=dev, dtype=torch.float32)
    check(lib.segan_reverb_fdl(_ptr(X), _ptr(bank.H), bank.H.shape[0], _ptr(ids), _ptr(bank.table),
                               bank.table.shape[0], _ptr(Y), rows, T, NB, M, _stream()),
          'reverb_fdl')
    if yt is None:
        yt = torch.empty((M, P), device=dev, dtype=torch.float32)
        check(lib.segan_reverb_inverse(_ptr(Y), _ptr(inv), _ptr(yt), M, _stream()),
              'reverb_inverse')
    y = torch.empty_like(x)
    prev_out = torch.empty(rows, device=dev, dtype=torch.float32)
    status = torch.empty(rows, device=dev, dtype=torch.int32)
    check(lib.segan_reverb_finish(_ptr(yt), _ptr(x), _ptr(lens), _ptr(prev), bank.H.shape[0],
                                  _ptr(ids), _ptr(bank.table), bank.table.shape[0], _ptr(y),
                                  _ptr(prev_out), _ptr(status), rows, T, NB, M, _stream()),
          'reverb_finish')
    return dict(xs=xs, X=X, Y=Y, yt=yt, y=y, prev=prev_out, status=status, dims=dims)


# ---------------------------------------------------------------------------------
# clipping, chunk removal and band limiting
# ---------------------------------------------------------------------------------
DISTORT_MAX_ROWS = 65535
CLIP_SILENT = _D['SEGAN_CLIP_ST_SILENT']     # status bits of clip_rows
CLIP_FACTOR = _D['SEGAN_CLIP_ST_FACTOR']
CHOP_MAX = _D['SEGAN_CHOP_MAX']              # chunks per row
CHOP_NOLEVEL = _D['SEGAN_CHOP_ST_NOLEVEL']   # status bit of chop_rows
FIR_MAX_K = _D['SEGAN_FIR_MAX_K']            # the longest one-sided filter
FIR_TILE = _D['SEGAN_FIR_TILE']              # outputs per workgroup
FIR_ID = _D['SEGAN_FIR_ST_ID']               # status bit of fir_rows


def _distort_rows(what, x, lengths, prev):
    """The checks the three ops share; (rows, T, lens)."""
    _chk(x, 'x', 2)
    rows, T = x.shape
    if rows == 0 or T == 0:
        raise ValueError('{}: empty input {}'.format(what, tuple(x.shape)))
    if rows > DISTORT_MAX_ROWS:
        raise ValueError('{}: 1 .. {} rows, got {}'.format(what, DISTORT_MAX_ROWS, rows))
    lens = None if lengths is None else _row_lengths(what, lengths, rows, T, x.device, True)
    _prev_arg(what, prev, rows, x.device)
    return rows, T, lens


def clip_rows(x, factors, lengths=None, prev=None):
    """Amplitude clipping of each row of x [rows, T] (fp32 CUDA) at a fraction of its own peak
    (DESIGN.md section 17): m = max |x[r, :len]|, thr = float32(float64(factor) * m), y = min(max(
    x, -thr), thr).  factors [rows]: host numbers in (0, 1] (anything else is refused here), or a
    CUDA float64 tensor (a value outside (0, 1] then gives status CLIP_FACTOR and the row
    unchanged).  lengths: host integers or a CUDA int32 tensor; samples past a row's length are
    copied.  prev (optional fp32 CUDA [rows]): the sample preceding each row, clamped like the row
    (it takes no part in m) and returned as info['prev'].  Returns (y, info) with info = dict(m,
    thr fp32 [rows], nclipped int32 [rows] (samples changed), status int32 [rows]: CLIP_SILENT (m
    == 0 or an empty row: unchanged) | CLIP_FACTOR).  No device-to-host copy."""
    rows, T, lens = _distort_rows('clip_rows', x, lengths, prev)

    def ok(t):
        f = t.to(torch.float64)
        if not bool(((f > 0) & (f <= 1)).all()):
            raise ValueError('clip_rows: factors must lie in (0, 1], got {}'.format(f.tolist()))

    f_d = _row_arg('clip_rows', 'factors', factors, (rows,), torch.float64, x.device, ok)
    y = torch.empty_like(x)
    prev_out = torch.empty_like(prev) if prev is not None else None
    m = torch.empty(rows, device=x.device, dtype=torch.float32)
    thr = torch.empty(rows, device=x.device, dtype=torch.float32)
    ncl = torch.empty(rows, device=x.device, dtype=torch.int32)
    status = torch.empty(rows, device=x.device, dtype=torch.int32)
    check(_lib.load().segan_clip_rows(_ptr(x), _ptr(lens), _ptr(prev), _ptr(f_d), rows, T, _ptr(y),
                                      _ptr(prev_out), _ptr(m), _ptr(thr), _ptr(ncl), _ptr(status),
                                      _stream()), 'clip_rows')
    info = dict(m=m, thr=thr, nclipped=ncl, status=status)
    if prev is not None:
        info['prev'] = prev_out
    return y, info


def chop_rows(x, q, c0, u, dur, lengths=None):
    """Up to CHOP_MAX chunks of each row of x [rows, T] (fp32 CUDA) zeroed where there is speech
    (DESIGN.md section 17).  q (fp64 CUDA [rows, T]) and c0 (fp64 CUDA [rows]) are the envelope and
    the threshold of `asl_p56_stages`: sample t < len is active when q[t] >= c0 (no hangover), n of
    them per row.  u [rows, C] in [0, 1) and dur [rows, C] >= 0 (samples; 0: an unused slot), host
    values or CUDA float64 / int32 tensors: slot c starts at the k-th active sample, k =
    min(floor(u n), n - 1), and zeroes [start, min(start + dur, len)).  Returns (y, info) with info
    = dict(starts int32 [rows, C] (-1: unused), nactive, nzeroed (size of the union), status int32
    [rows]: CHOP_NOLEVEL (c0 is NaN or nothing is active: the row unchanged, every start -1)).
    Integer arithmetic throughout; no device-to-host copy."""
    rows, T, lens = _distort_rows('chop_rows', x, lengths, None)
    _chk(q, 'q', None, torch.float64)
    if tuple(q.shape) != (rows, T):
        raise TypeError('chop_rows: q must be float64 [{}, {}]'.format(rows, T))
    c0 = _level_arg('chop_rows', 'c0', c0, rows)
    if q.device != x.device or c0.device != x.device:
        raise ValueError('chop_rows: tensors on different devices')
    ushape = tuple(u.shape) if hasattr(u, 'shape') else tuple(torch.as_tensor(u).shape)
    if len(ushape) != 2 or ushape[0] != rows or not 1 <= ushape[1] <= CHOP_MAX:
        raise ValueError('chop_rows: u must be [{}, C] with C from 1 to {}, got {}'.format(
            rows, CHOP_MAX, list(ushape)))
    C = ushape[1]

    def u_ok(t):
        f = t.to(torch.float64)
        if not bool(((f >= 0) & (f < 1)).all()):
            raise ValueError('chop_rows: u must lie in [0, 1), got {}'.format(f.tolist()))

    def dur_ok(t):
        if int(t.min()) < 0 or int(t.max()) >= 1 << 31:
            raise ValueError('chop_rows: dur must lie in 0 .. 2^31 - 1, got {}'.format(t.tolist()))

    u_d = _row_arg('chop_rows', 'u', u, (rows, C), torch.float64, x.device, u_ok)
    d_d = _row_arg('chop_rows', 'dur', dur, (rows, C), torch.int32, x.device, dur_ok)
    y = torch.empty_like(x)
    starts = torch.empty((rows, C), device=x.device, dtype=torch.int32)
    nact = torch.empty(rows, device=x.device, dtype=torch.int32)
    nzero = torch.empty(rows, device=x.device, dtype=torch.int32)
    status = torch.empty(rows, device=x.device, dtype=torch.int32)
    check(_lib.load().segan_chop_rows(_ptr(x), _ptr(lens), _ptr(q), _ptr(c0),
                                      _ptr(u_d), _ptr(d_d), rows, T, C, _ptr(y), _ptr(starts),
                                      _ptr(nact), _ptr(nzero), _ptr(status), _stream()),
          'chop_rows')
    return y, dict(starts=starts, nactive=nact, nzeroed=nzero, status=status)


def fir_rows(x, bank, K, ids, lengths=None, prev=None, out_dtype=None):
    """Zero-phase FIR filtering of each row of x [rows, T] (fp32 CUDA) with filter ids[r] of a bank
    of symmetric filters.  bank: fp64 CUDA [nf, Kmax + 1], the one-sided
    taps h[0 .. K[f]] with zeros after them, Kmax <= FIR_MAX_K; K: int32 CUDA [nf]; ids [rows]:
    host integers or a CUDA int32 tensor.  With xe[-1] = prev (0 without prev), xe = x on 0 ..
    len-1 and zero elsewhere: y[n] = h[0] xe[n] + sum_k h[k] (xe[n-k] + xe[n+k]), k ascending, in
    fp64 with every operation rounded on its own; y is zero from len on.  out_dtype: torch.float32
    (default; rounded once from the fp64 sum) or torch.float64.  Returns (y, info): info['prev'] =
    y[-1] ([rows], of out_dtype: what a pre-emphasis that follows needs), info['status'] int32
    [rows]: FIR_ID (the id is not in the bank: the row unchanged).  No device-to-host copy."""
    rows, T, lens = _distort_rows('fir_rows', x, lengths, prev)
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('fir_rows: out_dtype must be torch.float32 or torch.float64, got {}'.format(
            out_dtype))
    _chk(bank, 'bank', None, torch.float64)
    if bank.dim() != 2 or bank.shape[0] == 0 or bank.shape[1] == 0:
        raise TypeError('fir_rows: bank must be float64 [nf, Kmax + 1]')
    nf, kmax = bank.shape[0], bank.shape[1] - 1
    if kmax > FIR_MAX_K:
        raise ValueError('fir_rows: Kmax = {} exceeds {}'.format(kmax, FIR_MAX_K))
    _chk(K, 'K', None, torch.int32)
    if tuple(K.shape) != (nf,):
        raise TypeError('fir_rows: K must be int32 [{}]'.format(nf))
    if bank.device != x.device or K.device != x.device:
        raise ValueError('fir_rows: tensors on different devices')
    ids_d = _row_arg('fir_rows', 'ids', ids, (rows,), torch.int32, x.device,
                     lambda t: _fits_int32('fir_rows', 'ids', t))
    y = torch.empty((rows, T), device=x.device, dtype=out_dtype)
    prev_out = torch.empty(rows, device=x.device, dtype=out_dtype)
    status = torch.empty(rows, device=x.device, dtype=torch.int32)
    check(_lib.load().segan_fir_rows(_ptr(x), _ptr(lens), _ptr(prev), _ptr(bank), _ptr(K), nf, kmax,
                                     _ptr(ids_d), rows, T, _ptr(y), _RESAMPLE_DT[out_dtype],
                                     _ptr(prev_out), _ptr(status), _stream()), 'fir_rows')
    return y, dict(prev=prev_out, status=status)


# ---------------------------------------------------------------------------------
# whispered speech: noise-excited LPC resynthesis
# ---------------------------------------------------------------------------------
WHISPER_N = _D['SEGAN_WHISPER_N']            # frame
WHISPER_H = _D['SEGAN_WHISPER_H']            # hop
WHISPER_P = _D['SEGAN_WHISPER_P']            # order
WHISPER_WU = _D['SEGAN_WHISPER_WU']          # warm-up samples of the synthesis filter
WHISPER_SRATE = 16000
WHISPER_SILENT = _D['SEGAN_WHISPER_ST_SILENT']   # status bits of whisper_rows
WHISPER_TILT = _D['SEGAN_WHISPER_ST_TILT']
_whisper_tables_cache = {}
_whisper_ws = {}


def whisper_tables(lag_hz=120.0):
    """(window float64 [512], lagwin float64 [17]) on the host: the periodic Hann window w[m] = 0.5
    - 0.5 cos(2 pi m / 512) and the lag window g[l] = exp(-(2 pi lag_hz l / 16000)^2 / 2).
    Restated by scripts/whisper_oracle.py (hann, lag_window): keep them alike."""
    lag_hz = float(lag_hz)
    if not 0.0 <= lag_hz <= 1000.0:       # also refuses NaN
        raise ValueError('whisper: lag_hz must lie in 0 .. 1000 Hz, got {}'.format(lag_hz))
    m = np.arange(WHISPER_N, dtype=np.float64)
    lag = np.arange(WHISPER_P + 1, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * m / WHISPER_N),
            np.exp(-0.5 * (2.0 * np.pi * lag_hz * lag / WHISPER_SRATE) ** 2))


def _whisper_tables(device, lag_hz):
    """`whisper_tables` on `device`, uploaded once per device and lag_hz."""
    key = (device, float(lag_hz))
    if key not in _whisper_tables_cache:
        w, g = whisper_tables(lag_hz)
        pair = (torch.from_numpy(w).to(device), torch.from_numpy(g).to(device))
        torch.cuda.current_stream(device).synchronize()      # other streams use them next
        _whisper_tables_cache[key] = pair
    return _whisper_tables_cache[key]


def whisper_frames(T):
    return int(T) // WHISPER_H + 2


def _whisper_workspace(doubles, device):
    """The workspace of `whisper_rows` (86 MB at [300, 16384]), kept per (device, stream) and grown
    on demand like `_reverb_workspace`."""
    key = (device, _stream().value)
    ws = _whisper_ws.get(key)
    if ws is None or ws.numel() < doubles:
        ws = _whisper_ws[key] = torch.empty(doubles, device=device, dtype=torch.float64)
    return ws


def _whisper_seeds(what, seeds, rows, device):
    def ok(t):
        if t.numel() and int(t.min()) < 0:
            raise ValueError('{}: seeds must lie in 0 .. 2^63 - 1, got {}'.format(what, t.tolist()))

    return _row_arg(what, 'seeds', seeds, (rows,), torch.int64, device, ok)


def _whisper_args(what, x, seeds, tilts, lengths, prev):
    rows, T, lens = _distort_rows(what, x, lengths, prev)

    def tilt_ok(t):
        f = t.to(torch.float64)
        if not bool(((f >= 0) & (f < 1)).all()):
            raise ValueError('{}: tilts must lie in [0, 1), got {}'.format(what, f.tolist()))

    s_d = _whisper_seeds(what, seeds, rows, x.device)
    t_d = _row_arg(what, 'tilts', tilts, (rows,), torch.float64, x.device, tilt_ok)
    return rows, T, lens, s_d, t_d


def _whisper_out_dtype(what, out_dtype):
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('{}: out_dtype must be torch.float32 or torch.float64, got {}'.format(
            what, out_dtype))
    return out_dtype


def whisper_noise(seeds, j0, count, device=None):
    """u float64 [rows, count]: the samples j0 .. j0 + count - 1 of the excitation of each seed
    (host integers in 0 .. 2^63 - 1, or a CUDA int64 tensor): zero mean, unit variance, Philox4x32-10
    (DESIGN.md section 18).  -2^20 <= j0 <= 2^31."""
    if isinstance(seeds, torch.Tensor) and seeds.is_cuda:
        device = seeds.device
    elif device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    rows = int(seeds.numel()) if isinstance(seeds, torch.Tensor) else int(np.asarray(seeds).size)
    if rows == 0 or rows > DISTORT_MAX_ROWS:
        raise ValueError('whisper_noise: 1 .. {} seeds, got {}'.format(DISTORT_MAX_ROWS, rows))
    count = _int_arg(count, 'whisper_noise: count', 1, (1 << 31) - 1)
    j0 = _int_arg(j0, 'whisper_noise: j0', -(1 << 20), 1 << 31)
    s_d = _whisper_seeds('whisper_noise', seeds, rows, torch.device(device))
    u = torch.empty((rows, count), device=s_d.device, dtype=torch.float64)
    check(_lib.load().segan_whisper_noise(_ptr(s_d), j0, count, rows, _ptr(u), _stream()),
          'whisper_noise')
    return u


def whisper_lpc(r):
    """Levinson-Durbin with the whisper stage's guards on lags r (fp64 CUDA [..., 17]): dict(a [...,
    17], sigma [...], order int32 [...]).  The recursion stops at order m - 1, the higher
    coefficients zero, when k_m is not |k_m| < 1 or E has fallen to 2^-40 r[0]; r[0] <= 0: a = [1,
    0 ..], sigma = 0, order = 0."""
    _chk(r, 'r', None, torch.float64)
    if r.dim() < 1 or r.shape[-1] != WHISPER_P + 1 or r.numel() == 0:
        raise TypeError('whisper_lpc: r must be float64 [..., {}]'.format(WHISPER_P + 1))
    n = r.numel() // (WHISPER_P + 1)
    a = torch.empty_like(r)
    sigma = torch.empty(r.shape[:-1], device=r.device, dtype=torch.float64)
    order = torch.empty(r.shape[:-1], device=r.device, dtype=torch.int32)
    check(_lib.load().segan_whisper_lpc(_ptr(r), n, _ptr(a), _ptr(sigma), _ptr(order), _stream()),
          'whisper_lpc')
    return dict(a=a, sigma=sigma, order=order)


def whisper_stages(x, seeds, tilts, lengths=None, prev=None, lag_hz=120.0):
    """`whisper_rows` stage by stage through the library's separate entry points (tests, timing):
    dict(r, a [rows, F, 17], sigma, order [rows, F] with F = T // 256 + 2 (a row's own frames are
    the first len // 256 + 2), y64 [rows, T], prev64 [rows], peak, status, nsilent, minorder)."""
    rows, T, lens, s_d, t_d = _whisper_args('whisper_stages', x, seeds, tilts, lengths, prev)
    w, g = _whisper_tables(x.device, lag_hz)
    lib = _lib.load()
    dev, F = x.device, whisper_frames(T)
    r = torch.empty((rows, F, WHISPER_P + 1), device=dev, dtype=torch.float64)
    check(lib.segan_whisper_lags(_ptr(x), _ptr(lens), _ptr(prev), _ptr(w), _ptr(g), rows, T,
                                 _ptr(r), _stream()), 'whisper_lags')
    res = whisper_lpc(r)
    ws = torch.empty(rows * WHISPER_N * F, device=dev, dtype=torch.float64)
    y = torch.empty((rows, T), device=dev, dtype=torch.float64)
    prev_out = torch.empty(rows, device=dev, dtype=torch.float64)
    peak = torch.empty(rows, device=dev, dtype=torch.float64)
    status, nsilent, minorder = (torch.empty(rows, device=dev, dtype=torch.int32) for _ in range(3))
    check(lib.segan_whisper_synth(_ptr(x), _ptr(lens), _ptr(prev), _ptr(r), _ptr(res['a']),
                                  _ptr(res['sigma']), _ptr(res['order']), _ptr(s_d), _ptr(t_d),
                                  _ptr(w), rows, T, _ptr(ws), ws.numel(), _ptr(y),
                                  _RESAMPLE_DT[torch.float64], _ptr(prev_out), _ptr(peak),
                                  _ptr(status), _ptr(nsilent), _ptr(minorder), _stream()),
          'whisper_synth')
    res.update(r=r, y64=y, prev64=prev_out, peak=peak, status=status, nsilent=nsilent,
               minorder=minorder)
    return res


def whisper_rows(x, seeds, tilts, lengths=None, prev=None, out_dtype=None, lag_hz=120.0):
    """Whispered copies of the rows of x [rows, T] (fp32 CUDA, 16 kHz): noise-excited LPC
    resynthesis.  Frames of 512 at a hop of 256 under a periodic Hann window
    keep their order-16 spectral envelope (lag window of `lag_hz`) and their energy; the
    excitation is one continuous Philox noise sequence per row, seeds [rows] (host integers in 0 ..
    2^63 - 1 or a CUDA int64 tensor), tilted by e = (u[j] - tau u[j-1]) / sqrt(1 + tau^2) with tau
    = tilts [rows] in [0, 1): host numbers (anything else is refused here) or a CUDA float64 tensor
    (a value outside then gives status WHISPER_TILT and the row unchanged).  lengths: host integers
    or a CUDA int32 tensor; the output is zero from a row's length on.  prev (optional fp32 CUDA
    [rows]): the sample preceding each row.  If the result's peak exceeds 1 the row is divided by
    it.  out_dtype: torch.float32 (default; rounded once) or torch.float64.  Returns (y, info) with
    info = dict(prev (y[-1], of out_dtype), status int32 [rows]: WHISPER_SILENT (every frame is
    digital silence: unchanged) | WHISPER_TILT, nsilent int32 (silent frames), minorder int32 (the
    lowest order the recursion reached), peak float64 (before the guard)).  No device-to-host
    copy."""
    rows, T, lens, s_d, t_d = _whisper_args('whisper_rows', x, seeds, tilts, lengths, prev)
    out_dtype = _whisper_out_dtype('whisper_rows', out_dtype)
    w, g = _whisper_tables(x.device, lag_hz)
    lib = _lib.load()
    dev = x.device
    ws = _whisper_workspace(int(lib.segan_whisper_ws_doubles(rows, T)), dev)
    y = torch.empty((rows, T), device=dev, dtype=out_dtype)
    prev_out = torch.empty(rows, device=dev, dtype=out_dtype)
    peak = torch.empty(rows, device=dev, dtype=torch.float64)
    status, nsilent, minorder = (torch.empty(rows, device=dev, dtype=torch.int32) for _ in range(3))
    check(lib.segan_whisper_rows(_ptr(x), _ptr(lens), _ptr(prev), _ptr(s_d), _ptr(t_d), _ptr(w),
                                 _ptr(g), rows, T, _ptr(ws), ws.numel(), _ptr(y),
                                 _RESAMPLE_DT[out_dtype], _ptr(prev_out), _ptr(peak), _ptr(status),
                                 _ptr(nsilent), _ptr(minorder), _stream()), 'whisper_rows')
    return y, dict(prev=prev_out, status=status, nsilent=nsilent, minorder=minorder, peak=peak)


def rmsprop_step(p, g, sq, lr, alpha, eps):
    check(_lib.load().segan_rmsprop_step(_ptr(p), _ptr(g), _ptr(sq), lr, alpha, eps, p.numel(),
                                         _stream()), 'rmsprop_step')


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    check(_lib.load().segan_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), lr, beta1, beta2, eps,
                                      step, p.numel(), _stream()), 'adam_step')


def fill_(t, value):
    _chk(t, 't')
    check(_lib.load().segan_fill(_ptr(t), float(value), t.numel(), _stream()), 'fill')
    return t


def scale_(t, s):
    _chk(t, 't')
    check(_lib.load().segan_scale(_ptr(t), float(s), t.numel(), _stream()), 'scale')
    return t


# ---- data-parallel exchange through the C ABI (RCCL bound at run time) ------------------------
def comm_unique_id():
    """Rendezvous id (bytes) for `Comm`: create on rank 0, ship to the other ranks."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(lib.segan_comm_id_bytes())
    check(lib.segan_comm_unique_id(buf), 'comm_unique_id')
    return buf.raw


class Comm(object):
    """One RCCL communicator owned by libsegan_hip (segan_comm_init ... segan_comm_destroy): the
    data-parallel exchange of the GAN step without torch.distributed in the data path.  Creation
    is a collective over all ranks; the current CUDA device becomes the communicator's."""

    def __init__(self, world, rank, unique_id):
        lib = _lib.load()
        if len(unique_id) != lib.segan_comm_id_bytes():
            raise ValueError('Comm: unique id must be {} bytes'.format(lib.segan_comm_id_bytes()))
        h = ctypes.c_void_p()
        check(lib.segan_comm_init(ctypes.byref(h), int(world), int(rank), unique_id), 'comm_init')
        self._h, self.world, self.rank = h, int(world), int(rank)

    def _s(self, stream):
        return ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)

    def allreduce(self, t, scale=1.0, stream=None):
        """In-place sum over ranks of a contiguous fp32 CUDA tensor, then * scale."""
        _chk(t, 't')
        check(_lib.load().segan_allreduce(self._h, _ptr(t), t.numel(), float(scale), self._s(stream)),
              'allreduce')
        return t

    def broadcast(self, t, root=0, stream=None):
        _chk(t, 't')
        check(_lib.load().segan_broadcast(self._h, _ptr(t), t.numel(), int(root), self._s(stream)),
              'broadcast')
        return t

    def allgather(self, send, stream=None):
        """[world, *send.shape] <- every rank's `send`."""
        _chk(send, 'send')
        recv = torch.empty((self.world,) + tuple(send.shape), device=send.device, dtype=torch.float32)
        check(_lib.load().segan_allgather(self._h, _ptr(send), _ptr(recv), send.numel(),
                                          self._s(stream)), 'allgather')
        return recv

    def destroy(self):
        if self._h is not None:
            check(_lib.load().segan_comm_destroy(self._h), 'comm_destroy')
            self._h = None
