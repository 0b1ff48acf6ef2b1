"""Sweep of the GEMM, the STFT-loss stages, SSNR, the PCM kernels and spectral norm against float64.

segan_gemm, every stage of segan_stft.hip on its own, segan_ssnr, segan_pcm16_prep /
segan_pcm16_wave / segan_preemph_rows and segan_snorm_fwd / bwd run on the GPU and are compared with
a float64 reference on CPU copies of the same fp32 / int16 inputs: ``tests/emu_ops.py`` where it has
a counterpart that returns what the bar needs (stft_frames, stft_overlap_add, and the definitions
of powdb / powdb_bwd / stft_basis, which are restated here WITHOUT emu_ops' closing cast to fp32 and
pinned to emu_ops bit for bit), and restatements written in this module from the header comments of
the kernels and include/segan_hip.h otherwise (``ssnr_ref64``, ``pcm_x64`` / ``pcm_prep_ref``,
``preemph_rows_ref``; tests/test_frows.py pins the first two to the reference project's own
outputs in tests/golden/frows.pt without a GPU).

What the cases are built to reach
  segan_gemm, called through the C ABI (ops.gemm cannot pass ldc, flags or scratch freely)
    * five modes: fp32 atomics; SEGAN_GEMM_DETERMINISTIC with slabs in a 16-byte aligned scratch
      of segan_gemm_scratch_bytes (gemm_reduce_kernel); deterministic with scratch = NULL (what
      rv_gemm_blocked of segan_reverb.hip relies on); and the two fall-backs to the latter, a
      scratch one byte too small and one at base + 4 bytes, which also must leave the scratch
      untouched and give the bits of the NULL form;
    * beta0 in {1, 0} on a C pre-filled with 7.0 (overwrite must not see the 7, accumulate gives
      7 + ref); ldc in {N, N + 4, N + 1} with a sentinel in the columns N .. ldc of every row
      (hipMemset2DAsync and the ldc indexing of gemm_reduce_kernel);
    * the 128 x 128 kernel with 2 splits, with one chunk (K = 4 < 16: kchunks / 4 == 0), a ragged
      last chunk (K = 20), ragged tiles (130 x 72), many splits with a short last one (K = 2052);
      the 64 x 64 kernel below M * N = 4096, at K % 4 != 0, at 1 x 1 x 1, at K = 31 / 33 around
      its chunk of 32, and for an A whose base pointer is 4 bytes off a 16-byte boundary;
      ``fast_path`` restates the dispatch of segan_gemm.hip so that the table cannot drift;
    * all four operand layouts for every shape (a layout the 128 x 128 kernel cannot take, such as
      a row-contiguous A with M % 4 != 0, runs the 64 x 64 one and has to be right as well);
    * integer inputs from -8 .. 8: every product and partial sum is an integer below 2^24 for
      K <= 16384 (64 * 16384 = 2^20), so the result is exact in ANY summation order and a dropped,
      doubled or misplaced term cannot hide behind a rounding bar; also at the dense head's
      (300, 256, 16384) and (300, 16384, 256);
    * rows 0 .. 63 and 236 .. 299 of an M = 300 deterministic call without scratch are the bits of
      an M = 64 call on those rows.
  STFT stages at hop 160 / win 320: the smallest legal T = n_fft / 2 + 1 (320, 161), T = 162,
    T no multiple of the hop with 2 pad columns (512, 2000), no pad column and n_fft - win = 2
    (322, 480), (2048, 1025), and (2048, 16384) x 70 whose 2.3 M frame elements and 7.4 M bins reach
    the second trip of the capped loops of frames / powdb / powdb_bwd; (64, 33) with win 64, hop 1
    and (64, 40) with win 32, hop 100 for the general arguments.  powdb rows: re = im = 0,
    |S| = 1e-12 (far below eps), |S| = 1e3, im = 0 only; the pad columns of S hold NaN (never read)
    and those of dS and of the basis are exactly 0 in a NaN-filled buffer.  An odd n_fft is refused
    before any launch (one reflection cannot fold its largest padded index back: segan_stft.hip).
  segan_ssnr at 16 kHz, 8 kHz and 11025 Hz (window 331, hop 82: no multiple of 4), T giving 0, 1,
    1, 4 and many frames, 300 rows with deg == ref (every frame 35), a silent ref (every frame
    -10, overall -inf), both silent, and a row whose noise ramps through both clamps; a row of the
    300-row call is bit-equal to its single-row call.
  PCM kernels, bit for bit: int16 extremes, first mixed, coef 0.95 and 0, (1, 1) .. (70, 16384)
    (second grid trip), every int16 value through pcm16_wave, index = None and a permuted subset,
    T = 16385 (the grid-stride loop behind 64 x 256 threads), un-indexed rows keep a NaN sentinel.
    The kernels evaluate (2/65535)(pcm - 32767) + 1 and x - coef * xp as fused multiply-adds (one
    rounding where numpy has two); enumerating all 65536 values and, at coef 0.95, all 2^32
    (sample, previous sample) pairs on the CPU shows no pair whose fp32 result differs, so the
    bit-equality asked of pcm16_prep / pcm16_wave is a property of the kernel, not of the inputs
    drawn here.
  Spectral norm at 1 x 1 x 1, a single row, a single column, both dims, the Linear shape
    256 x 16384 (the largest row split of sn_matvec_t_kernel), with a NaN-filled workspace and a
    pre-filled dw over two calls.

Bars (u = 2^-24) and the largest value measured on an MI355X next to each
  * GEMM, integers: torch.equal.  GEMM, normal inputs: max_rel < TOL = 3e-5, the bar of
    tests/test_gpu_kernels.py (test_gemm_layouts)                  measured 1.7e-6 (128 x 256 x 2052)
  * stft_basis: one fp32 ulp at the entries' scale, 2^-23 / sqrt(n_fft): the kernel computes in
    double and rounds once                                     measured 0.35 of the bar
  * stft_frames, stft_overlap_add on integers, the adjoint identity on integers: torch.equal
  * stft_overlap_add, normal input: ``sum_tol`` of the pointwise sweep with m = 3 ceil(win / hop)
    terms per sample and no second pass                        measured 0.038 of the bar
  * powdb: |got - ref| <= 4.343 * 8u + 4u |ref|: three roundings in p + eps (4.343 = 10 / ln 10
    per unit of relative error), log10f good to 2 ulp, one rounding for the x 10
                                                               measured 0.73 of the bar
  * powdb_bwd: |got - ref| <= 8u |ref| per element (3.5 roundings in ddb * c / (p + eps) * re,
    doubled); exactly 0 where re resp. im is 0                 measured 0.61 of the bar
  * stft_pow_l1 with silent rows: the bars of test_stft_pow_l1_matches_torch_stft, loss 1e-5
    relative, gradient 5e-3 of its max                         measured 5.2e-8 and 2.2e-5
  * ssnr frames, mean, overall: |got - ref| <= 2^-23 max(1, |ref|): fp64 arithmetic rounded once
    to fp32; an infinite reference (log10 0) has to be met exactly
                                                               measured 0.67 of the bar (a mean)
  * PCM kernels: bit-equal
  * snorm: 2e-5 forward, 5e-5 backward, as test_snorm_fwd_bwd_matches_torch
                                                               measured 2.2e-6 and 4.2e-6

Outputs allocated inside ops.* come from torch.empty; ``poison`` hands the caching allocator a
NaN-filled block of the same size just before each such call.  Where this module calls the
library itself the output buffer is NaN-filled (or pre-filled as the case says) explicitly.
"""
import ctypes
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
TOL = 3e-5              # the bar of test_gemm_layouts in tests/test_gpu_kernels.py
NAN = float('nan')


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def ints(lo, hi, *shape, seed=0):
    """Integers lo .. hi (inclusive) as fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def dev(t):
    return None if t is None else t.to(DEV)


def place(t, off=0):
    """A device copy of t whose base pointer lies `off` floats past a 16-byte boundary."""
    if not off:
        return dev(t.contiguous())
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def poison(numel):
    """Best effort: leave a freed NaN block of the output's size for torch.empty to pick up."""
    t = torch.full((int(numel),), NAN, device=DEV, dtype=torch.float32)
    del t


def nan_buf(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def no_nan(*ts):
    for t in ts:
        assert not torch.isnan(t).any().item(), 'an output element was never stored'


def sum_tol(S, m, ns):
    """The derived bar of a sum (tests/test_gpu_pointwise_sweep.py): 2 (m + 16 + ns) 2^-24 sum|term|."""
    return 2 * (m + 16 + ns) * U * S


def report(what, value, bar=None):
    print('MEASURE {}: {:.4g}{}'.format(what, value, '' if bar is None else ' (bar {:g})'.format(bar)))


def check_bar(what, got, ref, bar):
    """|got - ref| <= bar elementwise (float64 tensors on the CPU); where the reference is infinite
    the output has to be that infinity.  Prints the worst |err| / bar."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    bar = torch.as_tensor(bar, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, what
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), what
    g, r, b = got[~inf], ref[~inf], bar[~inf]
    assert torch.isfinite(g).all(), what
    err = (g - r).abs()
    live = b > 0
    worst = (err[live] / b[live]).max().item() if live.any() else 0.0
    report(what + ' worst |err| / bar', worst, 1)
    assert (err <= b).all(), what
    return worst


# ---------------------------------------------------------------------------------------------
# 1. segan_gemm through the C ABI
# ---------------------------------------------------------------------------------------------
SENTINEL = -1234.5
MODES = ('atomics', 'slabs', 'no_scratch', 'scratch_short', 'scratch_misaligned')
DET_NOSPLIT = ('no_scratch', 'scratch_short', 'scratch_misaligned')
LAYOUTS = ((True, True), (True, False), (False, True), (False, False))

# (M, N, K, A's offset in floats, the kernel the k-contiguous layouts take)
GEMM_CASES = [
    (64, 64, 128, 0, 'fast'),        # 2 splits
    (64, 64, 4, 0, 'fast'),          # one chunk, kchunks / 4 == 0
    (64, 64, 20, 0, 'fast'),         # ragged chunk
    (130, 72, 132, 0, 'fast'),       # ragged tiles
    (128, 256, 2052, 0, 'fast'),     # many splits, the last one short
    (63, 65, 128, 0, 'generic'),     # M * N < 4096
    (1, 1, 1, 0, 'generic'),
    (3, 128, 1, 0, 'generic'),
    (37, 50, 33, 0, 'generic'),
    (37, 50, 31, 0, 'generic'),
    (64, 64, 126, 0, 'generic'),     # K % 4 != 0
    (64, 64, 128, 1, 'generic'),     # A at a base pointer 4 bytes off
]
GEMM_HEAD = [(300, 256, 16384, 0, 'fast'), (300, 16384, 256, 0, 'fast')]


def fast_path(M, N, K, a_k, b_k, a_off):
    """The dispatch of segan_gemm.hip restated: does this call take gemm128_kernel?"""
    lda, ldb = (K if a_k else M), (K if b_k else N)
    return ((a_k or M % 4 == 0) and (b_k or N % 4 == 0) and K % 4 == 0 and lda % 4 == 0
            and ldb % 4 == 0 and a_off == 0 and M * N >= 64 * 64)


def fast_splits(M, N, K):
    tiles = -(-M // 128) * -(-N // 128)
    kchunks = -(-K // 16)
    ns = max(1, min(-(-512 // tiles), kchunks // 4))
    kper = -(-kchunks // ns) * 16
    return -(-K // kper), kper


def test_gemm_case_table_reaches_the_paths_it_names():
    for (M, N, K, off, path) in GEMM_CASES + GEMM_HEAD:
        assert fast_path(M, N, K, True, True, off) == (path == 'fast'), (M, N, K, off)
    assert fast_splits(64, 64, 128) == (2, 64)
    assert fast_splits(64, 64, 4) == (1, 16)
    assert fast_splits(64, 64, 20) == (1, 32)
    ns, kper = fast_splits(128, 256, 2052)
    assert ns > 8 and 0 < 2052 - (ns - 1) * kper < kper
    # the scratch the library asks for is the slabs of that many splits (before the re-division)
    lib = _lib.load()
    assert lib.segan_gemm_scratch_bytes(64, 64, 128) == 2 * 64 * 64 * 4
    assert lib.segan_gemm_scratch_bytes(64, 64, 4) == 64 * 64 * 4


@functools.lru_cache(maxsize=4)
def gemm_inputs(M, N, K, kind):
    """A [M, K], B [K, N] on the CPU and the float64 product."""
    if kind == 'int':
        A, B = ints(-8, 8, M, K, seed=1), ints(-8, 8, K, N, seed=2)
    else:
        A, B = rnd(M, K, seed=1), rnd(K, N, seed=2)
    return A, B, A.double() @ B.double()


def gemm_operand(mat, k_contig, is_a, off=0):
    """(device tensor, stride over the row / column index, stride over k) of A [M, K] (is_a) or
    B [K, N]: k-contiguous storage is [M, K] resp. [N, K]."""
    rows_k = mat if is_a else mat.t()          # [M or N, K]
    if k_contig:
        return place(rows_k.contiguous(), off), rows_k.shape[1], 1
    return place(rows_k.t().contiguous(), off), 1, rows_k.shape[0]


class Scratch:
    """The (flags, scratch, scratch_bytes) of a mode; `intact` tells whether a scratch the library
    must not use still holds its fill."""
    def __init__(self, mode, M, N, K):
        self.mode = mode
        self.flags = 0 if mode == 'atomics' else 1          # SEGAN_GEMM_DETERMINISTIC
        self.ptr, self.nbytes, self.buf = None, 0, None
        if mode in ('slabs', 'scratch_short', 'scratch_misaligned'):
            need = _lib.load().segan_gemm_scratch_bytes(M, N, K)
            assert need > 0
            self.buf = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
            base = self.buf.data_ptr()
            assert base % 16 == 0
            self.ptr = ctypes.c_void_p(base + (4 if mode == 'scratch_misaligned' else 0))
            self.nbytes = need - 1 if mode == 'scratch_short' else need

    def intact(self):
        return self.mode == 'slabs' or self.buf is None or bool((self.buf == 0xA5).all().item())


def call_gemm(Ad, sam, sak, Bd, sbk, sbn, M, N, K, ldc, beta0, sc):
    """One segan_gemm into a C [M, ldc] pre-filled with 7.0 (columns N .. ldc: the sentinel)."""
    C = torch.empty((M, ldc), device=DEV, dtype=torch.float32)
    C[:, :N] = 7.0
    C[:, N:] = SENTINEL
    _lib.check(_lib.load().segan_gemm(ops._ptr(Ad), sam, sak, ops._ptr(Bd), sbk, sbn, ops._ptr(C),
                                      ldc, M, N, K, beta0, sc.flags, sc.ptr, sc.nbytes,
                                      ops._stream()), 'gemm')
    return C


def run_gemm_case(M, N, K, a_off, kind):
    """Every layout x mode x beta0 x ldc of one shape.  Returns the worst max_rel (normal inputs)."""
    A, B, ref = gemm_inputs(M, N, K, kind)
    ref_d = dev(ref)
    want = {1: ref_d, 0: ref_d + 7.0}
    den = {b: w.abs().max().item() or 1.0 for b, w in want.items()}
    scratch = {mode: Scratch(mode, M, N, K) for mode in MODES}
    worst = 0.0
    for a_k, b_k in LAYOUTS:
        Ad, sam, sak = gemm_operand(A, a_k, True, a_off)
        Bd, sbn, sbk = gemm_operand(B, b_k, False)
        for ldc in (N, N + 4, N + 1):
            for beta0 in (1, 0):
                bits = {}
                for mode in MODES:
                    sc = scratch[mode]
                    what = 'gemm {}x{}x{} a_off={} {} a_k={} b_k={} ldc={} beta0={} {}'.format(
                        M, N, K, a_off, kind, a_k, b_k, ldc, beta0, mode)
                    C = call_gemm(Ad, sam, sak, Bd, sbk, sbn, M, N, K, ldc, beta0, sc)
                    if ldc > N:
                        assert bool((C[:, N:] == SENTINEL).all().item()), what
                    assert sc.intact(), what
                    if kind == 'int':
                        assert torch.equal(C[:, :N].double(), want[beta0]), what
                    else:
                        e = (C[:, :N].double() - want[beta0]).abs().max().item() / den[beta0]
                        worst = max(worst, e)
                        assert e < TOL, (what, e)
                    if mode != 'atomics':
                        again = call_gemm(Ad, sam, sak, Bd, sbk, sbn, M, N, K, ldc, beta0, sc)
                        assert torch.equal(again, C), what
                        bits[mode] = C
                # a scratch the library cannot use means the form without scratch
                for mode in DET_NOSPLIT[1:]:
                    assert torch.equal(bits[mode], bits['no_scratch']), (M, N, K, a_k, b_k, ldc, mode)
    return worst


@pytest.mark.parametrize('M,N,K,a_off,path', GEMM_CASES + GEMM_HEAD)
def test_gemm_integers_are_exact_in_every_mode(M, N, K, a_off, path):
    run_gemm_case(M, N, K, a_off, 'int')


@pytest.mark.parametrize('M,N,K,a_off,path', GEMM_CASES)
def test_gemm_normal_inputs_in_every_mode(M, N, K, a_off, path):
    worst = run_gemm_case(M, N, K, a_off, 'normal')
    report('gemm normal {}x{}x{} a_off={} max_rel'.format(M, N, K, a_off), worst, TOL)


def test_gemm_without_scratch_rows_do_not_depend_on_the_batch():
    """The comment above rv_gemm_blocked (segan_reverb.hip): deterministic without scratch, an
    element depends only on its own row of A.  k-contiguous A, row-contiguous B."""
    M, N, K = 300, 256, 128
    A, B = rnd(M, K, seed=3), rnd(K, N, seed=4)
    Ad, Bd = dev(A), dev(B)
    sc = Scratch('no_scratch', M, N, K)
    full = call_gemm(Ad, K, 1, Bd, N, 1, M, N, K, N, 1, sc)
    assert max_rel(full, A.double() @ B.double()) < TOL
    for r0 in (0, 236):
        part = call_gemm(Ad[r0:r0 + 64], K, 1, Bd, N, 1, 64, N, K, N, 1, sc)
        assert torch.equal(part, full[r0:r0 + 64]), r0


# ---------------------------------------------------------------------------------------------
# 2. the STFT stages, each alone
# ---------------------------------------------------------------------------------------------
# (n_fft, T, B, win, hop)
STFT_GEOMS = [(320, 161, 3, 320, 160), (320, 162, 1, 320, 160), (512, 2000, 2, 320, 160),
              (322, 480, 2, 320, 160), (2048, 1025, 2, 320, 160), (2048, 16384, 70, 320, 160),
              (64, 33, 2, 64, 1), (64, 40, 2, 32, 100)]
EPS32 = float(np.float32(10e-20))       # the eps the kernels receive: a float argument


def geom_id(g):
    return 'nfft{}-T{}-B{}-win{}-hop{}'.format(*g)


def basis64(n_fft, win):
    """emu_ops.stft_basis without its cast: [win, 2 nbins] in float64."""
    nb = n_fft // 2 + 1
    left = (n_fft - win) // 2
    m = (torch.arange(nb).view(1, -1) * (left + torch.arange(win)).view(-1, 1)) % n_fft
    ang = 2 * math.pi * m.double() / n_fft
    return torch.cat((torch.cos(ang), -torch.sin(ang)), 1) / math.sqrt(n_fft)


def powdb64(S, nb, eps=EPS32):
    """emu_ops.powdb without its cast."""
    p = S[:, :nb].double() ** 2 + S[:, nb:2 * nb].double() ** 2
    return 10 * torch.log10(p + eps)


def powdb_bwd64(S, ddb, nb, eps=EPS32):
    """emu_ops.powdb_bwd without its cast or the pad columns: (dre, dim)."""
    re, im = S[:, :nb].double(), S[:, nb:2 * nb].double()
    g = ddb.double() * (20.0 / math.log(10.0)) / (re * re + im * im + eps)
    return g * re, g * im


def ola64(d, B, T, n_fft, hop, win):
    """emu_ops.stft_overlap_add without its cast."""
    idx = E._frame_index(T, n_fft, hop, win).reshape(-1)
    dx = torch.zeros(B, T, dtype=torch.float64)
    dx.index_add_(1, idx, d.double().view(B, -1))
    return dx


def test_stft_odd_n_fft_is_refused():
    """One reflection reaches 2 (T - 1); n_fft = win = 321 at T = 161 asks for index 321.  Both entry
    points refuse before they launch anything."""
    lib = _lib.load()
    for n_fft, win, hop, T in ((321, 321, 161, 161), (511, 320, 160, 320)):
        NF = 1 + T // hop
        x = torch.zeros(1, T, device=DEV)
        d = torch.zeros(NF, win, device=DEV)
        with pytest.raises(ValueError, match='odd n_fft'):
            ops.stft_frames(x, n_fft, hop, win)
        with pytest.raises(ValueError, match='odd n_fft'):
            ops.stft_overlap_add(d, 1, T, n_fft, hop, win)
        fr, dx = nan_buf(NF, win), nan_buf(1, T)
        assert lib.segan_stft_frames(ops._ptr(x), ops._ptr(fr), 1, T, n_fft, hop, win,
                                     ops._stream()) == -1          # SEGAN_EINVAL
        assert b'stft_frames: odd n_fft' in lib.segan_last_error()
        assert lib.segan_stft_overlap_add(ops._ptr(d), ops._ptr(dx), 1, T, n_fft, hop, win,
                                          ops._stream()) == -1
        assert b'stft_overlap_add: odd n_fft' in lib.segan_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(fr).all().item() and torch.isnan(dx).all().item()


@pytest.mark.parametrize('g', STFT_GEOMS, ids=geom_id)
def test_stft_basis(g):
    n_fft, _, _, win, _ = g
    nb, pitch = n_fft // 2 + 1, ops.stft_pitch(n_fft)
    assert pitch == _lib.load().segan_stft_pitch(n_fft) and pitch % 4 == 0 and 0 <= pitch - 2 * nb < 4
    bs = nan_buf(win, pitch)
    _lib.check(_lib.load().segan_stft_basis(ops._ptr(bs), n_fft, win, ops._stream()), 'stft_basis')
    no_nan(bs)
    bs = bs.cpu()
    assert pitch == 2 * nb or bool((bs[:, 2 * nb:] == 0).all())
    ref = basis64(n_fft, win)
    check_bar('stft_basis ' + geom_id(g), bs[:, :2 * nb], ref, 2.0 ** -23 / math.sqrt(n_fft))
    # emu_ops is the same definition, rounded
    emu = E.stft_basis(n_fft, win, 'cpu')
    assert emu.shape == bs.shape and torch.equal(emu[:, :2 * nb], ref.float())
    assert pitch == 2 * nb or bool((emu[:, 2 * nb:] == 0).all())


@pytest.mark.parametrize('g', STFT_GEOMS, ids=geom_id)
def test_stft_frames_and_overlap_add(g):
    n_fft, T, B, win, hop = g
    NF = 1 + T // hop
    # frames: a pure gather
    x = rnd(B, T, seed=21)
    poison(B * NF * win)
    fr = ops.stft_frames(dev(x), n_fft, hop, win)
    assert tuple(fr.shape) == (B * NF, win)
    assert torch.equal(fr.cpu(), E.stft_frames(x, n_fft, hop, win))
    # overlap-add on integers: exact
    d = ints(-5, 5, B * NF, win, seed=22)
    dg = dev(d)
    poison(B * T)
    dx = ops.stft_overlap_add(dg, B, T, n_fft, hop, win)
    assert tuple(dx.shape) == (B, T)
    assert torch.equal(dx.cpu(), E.stft_overlap_add(d, B, T, n_fft, hop, win))
    # <frames(x), d> == <x, ola(d)>, exactly on integers
    xi = ints(-8, 8, B, T, seed=23)
    poison(B * NF * win)
    fri = ops.stft_frames(dev(xi), n_fft, hop, win).cpu()
    assert (fri.double() * d.double()).sum().item() == (xi.double() * dx.cpu().double()).sum().item()
    # normal input: a sum of at most 3 ceil(win / hop) terms per sample, added by one thread
    dn = rnd(B * NF, win, seed=24)
    poison(B * T)
    dxn = ops.stft_overlap_add(dev(dn), B, T, n_fft, hop, win)
    no_nan(dxn)
    S = ola64(dn.abs(), B, T, n_fft, hop, win)
    check_bar('stft_overlap_add ' + geom_id(g), dxn, ola64(dn, B, T, n_fft, hop, win),
              sum_tol(S, 3 * -(-win // hop), 0))


@functools.lru_cache(maxsize=2)
def spectra(n_fft, rows):
    """S [rows, pitch] for powdb: normal spectra at the size of a unit-variance waveform's, rows
    0 .. 3 special, NaN in the pad columns (they are not part of the spectrum)."""
    nb, pitch = n_fft // 2 + 1, ops.stft_pitch(n_fft)
    S = rnd(rows, pitch, seed=31)
    phi = 2 * math.pi * torch.rand(2, nb, generator=torch.Generator().manual_seed(33))
    S[0, :] = 0.0                                              # re = im = 0
    S[1, :nb], S[1, nb:2 * nb] = 1e-12 * torch.cos(phi[0]), 1e-12 * torch.sin(phi[0])   # |S| = 1e-12
    S[2, :nb], S[2, nb:2 * nb] = 1e3 * torch.cos(phi[1]), 1e3 * torch.sin(phi[1])       # |S| = 1e3
    S[3, nb:2 * nb] = 0.0                                      # im = 0 only
    S[:, 2 * nb:] = NAN
    return S, rnd(rows, nb, seed=32)


@pytest.mark.parametrize('g', STFT_GEOMS, ids=geom_id)
def test_powdb_and_its_backward(g):
    n_fft, T, B, win, hop = g
    nb, pitch = n_fft // 2 + 1, ops.stft_pitch(n_fft)
    rows = max(B * (1 + T // hop), 8)
    S, ddb = spectra(n_fft, rows)
    Sg = dev(S)
    poison(rows * nb)
    db = ops.powdb(Sg, nb)
    assert tuple(db.shape) == (rows, nb)
    no_nan(db)
    ref = powdb64(S, nb)
    assert abs(ref[0, 0].item() + 190.0) < 1e-5 and abs(ref[1, 0].item() + 190.0) < 1e-3
    assert abs(ref[2, 0].item() - 60.0) < 1e-5
    check_bar('powdb ' + geom_id(g), db, ref, 4.343 * 8 * U + 4 * U * ref.abs())
    assert torch.equal(E.powdb(S, nb, EPS32), ref.float())
    # backward into a NaN-filled dS
    dS, ddb_g = nan_buf(rows, pitch), dev(ddb)
    _lib.check(_lib.load().segan_powdb_bwd(ops._ptr(Sg), ops._ptr(ddb_g), ops._ptr(dS), rows, nb,
                                           pitch, 10e-20, ops._stream()), 'powdb_bwd')
    no_nan(dS)
    dS = dS.cpu()
    assert pitch == 2 * nb or bool((dS[:, 2 * nb:] == 0).all())
    dre, dim = powdb_bwd64(S, ddb, nb)
    assert bool((dS[0, :2 * nb] == 0).all()) and bool((dS[3, nb:2 * nb] == 0).all())
    check_bar('powdb_bwd re ' + geom_id(g), dS[:, :nb], dre, 8 * U * dre.abs())
    check_bar('powdb_bwd im ' + geom_id(g), dS[:, nb:2 * nb], dim, 8 * U * dim.abs())
    emu = E.powdb_bwd(S, ddb, nb, EPS32)
    assert torch.equal(emu[:, :nb], dre.float()) and torch.equal(emu[:, nb:2 * nb], dim.float())
    # ops.powdb_bwd is the same call
    poison(rows * pitch)
    assert torch.equal(ops.powdb_bwd(Sg, ddb_g, nb).cpu(), dS)


def pow_db_torch(x, n_fft):
    st = torch.stft(x, n_fft=n_fft, hop_length=160, win_length=320, normalized=True,
                    window=torch.ones(320, dtype=x.dtype), return_complex=True)
    return 10 * torch.log10(st.abs() ** 2 + 10e-20)


@pytest.mark.parametrize('n_fft,T', [(320, 161), (512, 2000)])
def test_stft_pow_l1_with_silent_rows(n_fft, T):
    """The whole loss with an all-zero row in x and another in y, against torch.stft in float64 at
    the bars of test_stft_pow_l1_matches_torch_stft: every |X| of such a row is 0, where the dB
    derivative is 0 / eps."""
    from segan_pytorch_amd import losses
    B = 3
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 1, T, generator=g) * 2 - 1
    y = (x + 0.3 * torch.randn(B, 1, T, generator=g)).clamp(-1, 1)
    x[0] = 0.0
    y[1] = 0.0
    xd = x.double().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(pow_db_torch(xd.squeeze(1), n_fft),
                                      pow_db_torch(y.double().squeeze(1), n_fft))
    ref.backward()
    xg = dev(x).requires_grad_(True)
    loss = losses.stft_pow_l1(xg, dev(y), n_fft)
    loss.backward()
    assert math.isfinite(loss.item()) and torch.isfinite(xg.grad).all().item()
    assert bool((xg.grad[0] == 0).all().item()) and bool((xd.grad[0] == 0).all().item())
    eloss = abs(loss.item() - ref.item()) / abs(ref.item())
    egrad = max_rel(xg.grad, xd.grad)
    report('stft_pow_l1 silent rows n_fft={} T={} loss rel err'.format(n_fft, T), eloss, 1e-5)
    report('stft_pow_l1 silent rows n_fft={} T={} grad max_rel'.format(n_fft, T), egrad, 5e-3)
    assert eloss < 1e-5
    assert egrad < 5e-3


# ---------------------------------------------------------------------------------------------
# 3. segmental SNR
# ---------------------------------------------------------------------------------------------
def ssnr_geometry(srate):
    win = int(math.floor(30.0 * srate / 1000.0 + 0.5))
    return win, win // 4


def ssnr_ref64(ref, deg, srate=16000, eps=1e-10):
    """The definition in the header comment of segan_audio.hip in numpy float64:
    (overall[rows], mean[rows], frames[rows, nf])."""
    ref, deg = np.asarray(ref, dtype=np.float64), np.asarray(deg, dtype=np.float64)
    rows, T = ref.shape
    win, skip = ssnr_geometry(srate)
    nf = max(int(T / skip - win / skip), 0)
    k = np.arange(1, win + 1, dtype=np.float64)
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * k / (win + 1)))
    seg = np.empty((rows, nf))
    for f in range(nf):
        c = ref[:, f * skip:f * skip + win] * w
        p = deg[:, f * skip:f * skip + win] * w
        seg[:, f] = 10.0 * np.log10((c * c).sum(1) / (((c - p) ** 2).sum(1) + eps) + eps)
    seg = np.clip(seg, -10.0, 35.0)
    with np.errstate(divide='ignore'):
        overall = 10.0 * np.log10((ref * ref).sum(1) / (((ref - deg) ** 2).sum(1) + 10e-20))
    mean = seg.mean(1) if nf else np.zeros(rows)
    return overall, mean, seg


SSNR_ROWS = 300


def ssnr_lengths(srate):
    win, skip = ssnr_geometry(srate)
    return [win + skip - 1, win + skip, win + skip + 1, 2 * win, 16384], [0, 1, 1, 4, None]


@functools.lru_cache(maxsize=2)
def ssnr_inputs(srate, T):
    """300 rows: 0 deg == ref; 1 silent ref; 2 both silent; 3 noise ramping from -80 dB to +40 dB
    of the signal along the row; the others a signal with noise 10 dB .. 30 dB below it."""
    ref = 0.1 * rnd(SSNR_ROWS, T, seed=41)
    noise = rnd(SSNR_ROWS, T, seed=42)
    level = 10.0 ** (-(10.0 + 20.0 * torch.rand(SSNR_ROWS, 1, generator=torch.Generator().manual_seed(43))) / 20.0)
    deg = ref + 0.1 * level.float() * noise
    deg[0] = ref[0]
    ref[1] = 0.0
    ref[2] = 0.0
    deg[2] = 0.0
    ramp = 10.0 ** (torch.linspace(-80.0, 40.0, T) / 20.0)
    deg[3] = ref[3] + 0.1 * ramp * noise[3]
    return ref, deg, ssnr_ref64(ref.numpy(), deg.numpy(), srate)


@pytest.mark.parametrize('srate', (16000, 8000, 11025))
def test_ssnr(srate):
    lib = _lib.load()
    win, skip = ssnr_geometry(srate)
    if srate == 11025:
        assert (win, skip) == (331, 82)
    worst = 0.0
    for T, nf_want in zip(*ssnr_lengths(srate)):
        ref, deg, (overall, mean, seg) = ssnr_inputs(srate, T)
        nf = seg.shape[1]
        assert nf == lib.segan_ssnr_frames(T, srate) and (nf_want is None or nf == nf_want)
        # what the rows were built for, on the reference side
        if nf:
            assert (seg[0] == 35.0).all() and (seg[1] == -10.0).all() and (seg[2] == -10.0).all()
        assert np.isfinite(overall[0]) and overall[0] > 100.0
        assert overall[1] == -np.inf and overall[2] == -np.inf
        if T == 16384:
            assert seg[3, 0] == 35.0 and seg[3, -1] == -10.0
            assert ((seg[3] > -9.0) & (seg[3] < 34.0)).sum() >= 10
            assert ((seg[4:] > -10.0) & (seg[4:] < 35.0)).all()
        rg, dg = dev(ref), dev(deg)
        poison(SSNR_ROWS * max(nf, 1))
        snr, mseg, frames = ops.ssnr(rg, dg, srate)
        assert tuple(frames.shape) == (SSNR_ROWS, nf) and tuple(snr.shape) == (SSNR_ROWS,)
        no_nan(frames, mseg)
        what = 'ssnr srate={} T={}'.format(srate, T)
        bar = lambda r: 2.0 ** -23 * np.maximum(1.0, np.abs(np.where(np.isinf(r), 0.0, r)))
        if nf:
            worst = max(worst, check_bar(what + ' frames', frames, torch.from_numpy(seg), bar(seg)))
        else:
            assert frames.numel() == 0 and bool((mseg == 0).all().item())
        worst = max(worst, check_bar(what + ' mean', mseg, torch.from_numpy(mean), bar(mean)))
        worst = max(worst, check_bar(what + ' overall', snr, torch.from_numpy(overall), bar(overall)))
        # a row does not depend on its batch
        for r in (0, 1, 2, 3, 150, SSNR_ROWS - 1):
            s1, m1, f1 = ops.ssnr(rg[r:r + 1].contiguous(), dg[r:r + 1].contiguous(), srate)
            assert torch.equal(f1[0], frames[r]), (what, r)
            # (-inf == -inf holds for torch.equal)
            assert torch.equal(s1[0], snr[r]) and torch.equal(m1[0], mseg[r]), (what, r)
    report('ssnr srate={} worst |err| / bar'.format(srate), worst, 1)


# ---------------------------------------------------------------------------------------------
# 4. the PCM input kernels, bit for bit
# ---------------------------------------------------------------------------------------------
def pcm_x64(pcm):
    """int16 -> the min-max normalised wave in float64, as numpy evaluates it."""
    return (2.0 / 65535.0) * (np.asarray(pcm).astype(np.float64) - 32767.0) + 1.0


def pcm_preemph64(x, coef, first=False):
    """y[n] = x[n] - coef x[n-1] along the last axis of x [..., T + 1] (x[..., 0]: the sample before
    the slice) in float64: [..., T]; y[0] = x[0] of the slice for a slice that starts its wav."""
    y = x[..., 1:] - coef * x[..., :-1]
    first = np.asarray(first, dtype=bool)
    y[..., 0] = np.where(first, x[..., 1], y[..., 0])
    return y


def pcm_prep_ref(pcm, first, coef):
    """(clean, noisy) fp32 [B, T] of pcm int16 [B, 2, T + 1], first [B]."""
    y = pcm_preemph64(pcm_x64(pcm), coef, np.asarray(first, dtype=bool)[:, None]).astype(np.float32)
    return y[:, 0], y[:, 1]


def preemph_rows_ref(x, prev, first, coef):
    """fp32 wave x [n, T] with prev [n] -> float32(double(x[t]) - coef double(x[t-1]))."""
    xd = np.concatenate((np.asarray(prev, dtype=np.float64)[:, None], np.asarray(x, dtype=np.float64)), 1)
    return pcm_preemph64(xd, coef, np.asarray(first, dtype=bool)).astype(np.float32)


def pcm_block(B, T, seed):
    """int16 [B, 2, T + 1] over the full range with the extremes and 0 planted, clean != noisy."""
    g = torch.Generator().manual_seed(seed)
    pcm = torch.randint(-32768, 32768, (B, 2, T + 1), generator=g, dtype=torch.int32).to(torch.int16)
    flat = pcm.view(-1)
    plant = [-32768, 32767, 0, 32767, -32768]
    for k, v in enumerate(plant[:flat.numel()]):
        flat[k] = v
    for k, v in enumerate(plant[:flat.numel()]):
        flat[flat.numel() - 1 - k] = v
    return pcm


@pytest.mark.parametrize('coef', (0.95, 0.0))
@pytest.mark.parametrize('B,T', ((1, 1), (3, 7), (70, 16384)))
def test_pcm16_prep_is_bit_exact(B, T, coef):
    pcm = pcm_block(B, T, seed=51)
    first = (torch.arange(B) % 3 == 0).to(torch.uint8)
    if B > 1:
        assert first.min() == 0 and first.max() == 1 and not torch.equal(pcm[:, 0], pcm[:, 1])
    want_c, want_n = pcm_prep_ref(pcm.numpy(), first.numpy(), coef)
    poison(B * T)
    poison(B * T)
    clean, noisy = ops.pcm16_prep(pcm.to(DEV), first.to(DEV), coef)
    assert clean.dtype == torch.float32 and tuple(clean.shape) == (B, T) == tuple(noisy.shape)
    assert np.array_equal(clean.cpu().numpy(), want_c)
    assert np.array_equal(noisy.cpu().numpy(), want_n)


def run_pcm16_wave(pcm, index):
    B, T = pcm.shape[0], pcm.shape[2] - 1
    x = pcm_x64(pcm.numpy()).astype(np.float32)[:, 0]            # the clean rows [B, T + 1]
    sel = list(range(B)) if index is None else index
    poison(len(sel) * T)
    wave, prev = ops.pcm16_wave(pcm.to(DEV), index)
    assert tuple(wave.shape) == (len(sel), T) and tuple(prev.shape) == (len(sel),)
    assert np.array_equal(wave.cpu().numpy(), x[sel, 1:])
    assert np.array_equal(prev.cpu().numpy(), x[sel, 0])


@pytest.mark.parametrize('T', (1, 7, 16384 + 1))
def test_pcm16_wave_is_bit_exact(T):
    pcm = pcm_block(7, T, seed=52)
    run_pcm16_wave(pcm, None)
    run_pcm16_wave(pcm, [5, 0, 3])
    run_pcm16_wave(pcm, [6])


def test_pcm16_wave_every_int16_value():
    """All 65536 sample values in one row (and the first of them as prev)."""
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    row = torch.cat((every[:1], every))                        # [T + 1], T = 65536
    pcm = torch.stack((row, row.flip(0))).unsqueeze(0).contiguous()
    run_pcm16_wave(pcm, None)


@pytest.mark.parametrize('coef', (0.95, 0.0))
@pytest.mark.parametrize('T', (1, 7, 16384 + 1))
def test_preemph_rows_is_bit_exact(T, coef):
    B = 7
    first = torch.tensor([0, 1, 0, 1, 0, 0, 1], dtype=torch.uint8)
    for index in (None, [5, 0, 3], [3, 6]):
        sel = list(range(B)) if index is None else index
        n = len(sel)
        g = torch.Generator().manual_seed(53 + n)
        x = torch.rand(n, T, generator=g) * 2 - 1
        prev = torch.rand(n, generator=g) * 2 - 1
        want = preemph_rows_ref(x.numpy(), prev.numpy(), first.numpy()[sel], coef)
        out = nan_buf(B, T)
        got = ops.preemph_rows(dev(x), dev(prev), first.to(DEV), out, coef, index)
        assert got is out
        got = out.cpu().numpy()
        for k, b in enumerate(sel):
            assert np.array_equal(got[b], want[k]), (index, k, b)
            if first[b]:
                assert got[b, 0] == x[k, 0].item()
            if coef == 0.0:
                assert np.array_equal(got[b], x[k].numpy())
        for b in set(range(B)) - set(sel):
            assert np.isnan(got[b]).all(), (index, b)            # rows that are not indexed are not written


# ---------------------------------------------------------------------------------------------
# 5. spectral normalisation: the edges of the grid of test_snorm_fwd_bwd_matches_torch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dim', [((1, 1, 1), 0), ((1, 5, 3), 0), ((1, 5, 3), 1), ((5, 1, 3), 1),
                                       ((256, 16384), 0), ((3, 70, 31), 1)])
@pytest.mark.parametrize('power_iteration', [True, False])
def test_snorm_edges(shape, dim, power_iteration):
    """As test_snorm_fwd_bwd_matches_torch (tests/test_gpu_kernels.py), through the C ABI so that
    the workspace is a NaN-filled block; dw is pre-filled and the backward called twice."""
    import torch.nn.functional as F
    lib = _lib.load()
    w = rnd(*shape, seed=1) * 0.3
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

    A, Bd, K = ops._sn_view(w, dim)
    nws = lib.segan_snorm_ws_floats(A, Bd, K, dim)
    assert nws > 0
    wg, gg = dev(w), dev(g)
    ug, vg = u0.float().to(DEV), v0.float().to(DEV)
    w_sn, sig, ws = nan_buf(*shape), nan_buf(1), nan_buf(nws)
    _lib.check(lib.segan_snorm_fwd(ops._ptr(wg), ops._ptr(ug), ops._ptr(vg), ops._ptr(w_sn),
                                   ops._ptr(sig), ops._ptr(ws), A, Bd, K, dim,
                                   1 if power_iteration else 0, 1e-12, ops._stream()), 'snorm_fwd')
    no_nan(w_sn, sig, ug, vg)
    what = 'snorm {} dim={} power_iteration={}'.format(shape, dim, power_iteration)
    efwd = max(max_rel(ug, u), max_rel(vg, v), abs(sig.item() - sigma.item()) / abs(sigma.item()),
               max_rel(w_sn, w_sn_ref))
    report(what + ' forward', efwd, 2e-5)
    assert max_rel(ug, u) < 2e-5 and max_rel(vg, v) < 2e-5
    assert abs(sig.item() - sigma.item()) < 2e-5 * abs(sigma.item())
    assert max_rel(w_sn, w_sn_ref) < 2e-5
    if not power_iteration:
        assert torch.equal(ug.cpu(), u0.float()) and torch.equal(vg.cpu(), v0.float())
    # ops.snorm_fwd is the same call with a workspace from torch.empty
    u2, v2 = u0.float().to(DEV), v0.float().to(DEV)
    poison(nws)
    w_sn2, sig2 = ops.snorm_fwd(wg, u2, v2, dim, power_iteration)
    assert max_rel(w_sn2, w_sn_ref) < 2e-5 and max_rel(u2, u) < 2e-5 and max_rel(v2, v) < 2e-5
    # backward: accumulates, twice
    dw = torch.full(shape, 0.25, device=DEV)
    ws.fill_(NAN)
    _lib.check(lib.segan_snorm_bwd(ops._ptr(gg), ops._ptr(wg), ops._ptr(ug), ops._ptr(vg),
                                   ops._ptr(sig), ops._ptr(dw), ops._ptr(ws), A, Bd, K, dim,
                                   ops._stream()), 'snorm_bwd')
    dw1 = dw.clone()
    ws.fill_(NAN)
    _lib.check(lib.segan_snorm_bwd(ops._ptr(gg), ops._ptr(wg), ops._ptr(ug), ops._ptr(vg),
                                   ops._ptr(sig), ops._ptr(dw), ops._ptr(ws), A, Bd, K, dim,
                                   ops._stream()), 'snorm_bwd')
    no_nan(dw1, dw)
    ebwd = max(max_rel(dw1 - 0.25, wd.grad), max_rel(dw.double() - dw1.double(), wd.grad),
               max_rel(dw - 0.25, 2 * wd.grad))
    report(what + ' backward', ebwd, 5e-5)
    assert max_rel(dw1 - 0.25, wd.grad) < 5e-5
    assert max_rel(dw.double() - dw1.double(), wd.grad) < 5e-5
    assert max_rel(dw - 0.25, 2 * wd.grad) < 5e-5
