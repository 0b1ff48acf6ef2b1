"""The launch plans of the contractions over grid sizes, bit for bit against fp64.

conv1d_fwd, conv1d_dgrad, deconv1d_fwd, deconv1d_dgrad (fp32, bf16, bf16x3) and the fp32 weight
gradient plan their launches from ``G = segan_grid_slots(occ)`` = 256 x resident workgroups per CU
minus the reserve (``ops.set_reserved_slots``), floored at 64: one workgroup per tile, a persistent
grid striding over whole tiles, stream-K (``sk_nfull`` whole tiles, the rest cut into pieces of
``sk_units`` chunks: TileIter, two slabs per workgroup, corr_fixup_kernel), and for wgrad2_kernel
the split count and the chunks per split.  The other modules run these plans at a reserve of 0 only
(G = 256 occ, a multiple of 8) and with random inputs behind a bar of 3e-5 of max|ref|.  Here the
RESERVE varies: every case of tests/plan_sweep_cases.py runs under each of 0, 5, 77, 509 and 512
(the table of grids is in that module's docstring), set through ``ops.set_reserved_slots`` inside
the process and put back after every test.

Exact leg.  The value sets of tests/test_gpu_src_sweep.py (small integers and quarter-integers; the
unmarked test below asserts its condition per case), so every partial sum in any cut order is an
fp32 number, and per case x reserve x precision: the stream's stream-K scratch and call scratch
are filled with NaN bytes, a freed NaN block of the output's size is left for torch.empty, the call
goes through ``ops``, the result must be ``torch.equal`` to fp64, the launch record must equal the
restated planner (kernel id, workgroups, tiles, whole tiles, units; for the weight gradient tiles,
splits, chunks per split), and a second call must give the same bits and the same record.  The
weight gradient runs in the default atomic mode and in deterministic mode (dw = pre-fill + ref after
one call, + 2 ref after two; in deterministic mode a repeat from the same pre-fill is bit-equal,
which the random-valued leg asserts where it is not a consequence of exactness).

The corr record does not state the occupancy the planner used.  A record must equal the restatement
for at least one occupancy of 1 .. 4, and all records of one kernel instance (kernel, form, tile,
chunk length, LDS window) must agree on one: a grid that no occupancy explains fails.  A classic
record (one workgroup per tile) fits every occupancy: there the record check says no more than
workgroups = tiles = the restated tile count, and the instance's occupancy is fixed by its cut cases.

Classes (per fp32 form F = conv1d_fwd / deconv1d_dgrad, T = deconv1d_fwd / conv1d_dgrad):
  1 classic, one workgroup per tile          2 persistent grid, fewer workgroups than tiles, a
  3 stream-K, no whole tiles                   partial last round, no cut
  4 stream-K behind whole tiles              5 stream-K, a piece spanning two tiles
  6 stream-K with paired channels (F form, K = 31, even N, corr2_kernel), and 6.1: the pairing moved
    the cut to an even chunk                 7 stream-K beside dead tiles (deconv1d_dgrad, dx0 NULL)
  8 a grid that is no multiple of 8 in class 2 (8.2) and in class 4 (8.4)
bf16 and bf16x3 (corr_bf2_kernel): 3, 4, 5.  Weight gradient: three or more split counts of one
geometry over the reserves, and a split length that does not divide the chunk count.  The unmarked
tests assert that table x reserves reaches every class at EVERY occupancy of 1 .. 4; the closing GPU
test classifies the records this device produced and fails, naming the class, if one is missing.

Scratch leg (C ABI, as tests/test_gpu_dense_sweep.py): one F and one T stream-K case with scratch
NULL and one float short of G 2 MB NB (the launch must stay classic), of exactly that size with a
NaN guard behind it (stream-K; the guard must be untouched) and of the full size; all four exact.

Random-valued leg: the cases marked ``rand`` under reserves 77 and 512 against fp64 at the bars of
test_gpu_kernels.py: 3e-5 (fp32), 5e-5 (bf16x3), 2e-2 (bf16) of max|ref|.

Blocked fp32 (``ops.set_accumulation('blocked')``, corr2_kernel's stride-4 128-row instances)
runs the same cases and must reach 3, 4, 5 and 6.1 as well.

Observed on an MI355X (the closing test prints this; first record per class; workgroups / tiles /
whole tiles / units).  Occupancy: corr2_kernel F form 4, T form 3 (stride 2: 2), blocked 2;
corr_kernel 3; corr_bf2_kernel bf16 3, bf16x3 2; wgrad2_kernel 4.
  F  1 p_f_classic r0 30/30/30/0       2 p_f_persist r0 1024/2051/2051/0   3 p_f_pair_72 r0 1024/72/0/2
     4, 8.4 p_f_600 r509 515/600/515/2   5 p_f_odd_100 r509 515/100/0/2      6, 6.1 p_f_pair_72 r0 1024/72/0/2
     7 p_x_dead_72 r0 1024/72/0/2        8.2 p_f_persist r5 1019/2051/2051/0
  T  1 p_t_classic r0 30/30/30/0       2 p_t_persist r0 768/2051/2051/0    3 p_t_72 r0 768/72/0/1
     4, 8.4 p_t_600 r509 259/600/518/6   5 p_t_72 r509 259/72/0/3            8.2 p_t_persist r5 763/2051/2051/0
  bf16    3 p_f_bf_80 r0 768/80/0/1    4 p_t_600 r509 259/600/518/3        5 p_f_bf_80 r509 259/80/0/3
  bf16x3  3, 5 p_f_pair_72 r0 512/72/0/3   4 p_f_pair_72 r509 64/72/64/2
  blocked 3 p_f_pair_72 r0 512/72/0/2  4, 6.1 p_f_pair_72 r509 64/72/64/2   5 p_f_odd_100 r0 512/100/0/2
  wgrad p_w_2tiles (88 chunks), reserve: splits x chunks per split = 0, 5: 11 x 8; 77: 10 x 9 (last
  split 7); 509, 512: 6 x 15 (last split 13).  p_w_s2 (100 chunks): 7 x 15 and 12 x 9.
The sweep found no defect in the planners or kernels.

Size and time: 392 GPU tests (340 exact, 48 random-valued, 2 on scratch, the two closing ones) and
10 CPU tests.  Measured on an MI355X: 3.0 s for the whole module (pytest's total, fp64 references
included; the slowest test 0.7 s), against 2.1 s for the src sweep's 414 tests.
"""
import contextlib
import ctypes

import pytest
import torch

import plan_sweep_cases as P
import test_gpu_src_sweep as SW
from segan_pytorch_amd import _lib, ops

gpu = pytest.mark.gpu
DEV = SW.DEV
dev, same, to_src, poison, mode = SW.dev, SW.same, SW.to_src, SW.poison, SW.mode
# of max|ref| (test_gpu_kernels.py: TOL, PREC_TOL); blocked fp32 is held to the fp32 bar
BARS = {'fp32': 3e-5, 'det': 3e-5, 'blocked': 3e-5, 'bf16x3': 5e-5, 'bf16': 2e-2}

OCC = {}            # kernel instance -> the occupancies every record of it agrees with
SEEN = {}           # (group, class) -> (case, precision, reserve, record) that reached it first
WSEEN = {}          # wgrad case -> {reserve: (occ, splits, chunks per split, chunks)}
RAN = set()         # ids of the exact-leg tests that were started in this session
STATE = {}


# ---------------------------------------------------------------------------------------------
# the table and the restated planners (no GPU)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', list(P.TABLES))
def test_plan_table_is_exact(kind):
    worst = 0.0
    for c in P.TABLES[kind]:
        worst = max(worst, P.check_exact(c))
    print('{}: largest |contraction| = {:.3g} units (bound 2^24 = {:.3g})'.format(kind, worst, 2.0 ** 24))


@pytest.mark.parametrize('occ', P.OCCS)
def test_table_reaches_every_class_at_this_occupancy(occ):
    seen = set()
    for c in P.CORR:
        for prec in P.precisions(c):
            for r in P.RESERVES:
                ln, rec = P.plan_corr(c, prec, occ, r)
                seen |= {(P.group(c, prec), k) for k in P.classify(ln, rec)}
    assert not P.missing(seen), P.missing(seen)
    # weight gradient: one geometry with three or more split counts, one uneven last split
    plans = {c.name: [P.wgrad2_plan(w.tiles, w.nch, P.grid_slots(occ, r)) + (w.nch,) for r in P.RESERVES]
             for c in P.WGRAD for w in [P.launch_wgrad2(c)]}
    assert any(len({s for s, _, _ in pl}) >= 3 for pl in plans.values()), plans
    assert any(s > 1 and n % cps for pl in plans.values() for s, cps, n in pl), plans


def test_reserves_and_planner_invariants():
    r = P.RESERVES
    assert 0 in r and 512 in r and sum(1 for v in r if v % 8) >= 2
    # the setter clamps at 512: this is as far down as occupancy 3 and 4 go
    assert [P.grid_slots(o, 512) for o in P.OCCS] == [64, 64, 256, 512]
    # what the kernels rely on: a piece never holds more than two tiles' chunks (two slabs per
    # workgroup), the pieces cover the cut tiles, paired cuts are even, the slabs fit the scratch
    for c in P.CORR:
        for prec in P.precisions(c):
            for occ in P.OCCS:
                for res in r:
                    ln, rec = P.plan_corr(c, prec, occ, res)
                    u, wg = rec['streamk_units'], rec['workgroups']
                    if not u:
                        continue
                    total = (rec['tiles'] - rec['tiles_whole']) * ln.nch
                    assert 0 < u <= ln.nch and u * wg >= total, (c.name, prec, occ, res, rec)
                    assert not ln.pair_cuts or (u % 2 == 0 and ln.nch % 2 == 0), (c.name, rec)
                    assert wg * 2 * ln.slab <= P.SCRATCH_FLOATS and rec['tiles_whole'] % wg == 0


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def reserve_guard():
    """Remembers the reserve the module started with and puts it back whatever happens."""
    start = ops.set_reserved_slots(0)
    ops.set_reserved_slots(start)
    STATE['start'] = start
    try:
        yield start
    finally:
        ops.set_reserved_slots(start)


@contextlib.contextmanager
def reserved(n):
    prev = ops.set_reserved_slots(n)
    try:
        yield
    finally:
        ops.set_reserved_slots(prev)


def poison_scratch():
    """NaN bytes over this stream's stream-K scratch and over the call scratch (the packed bf16
    operand and its slabs; the weight gradient's materialised lo and partial tiles)."""
    ops._scratch()
    for d in (ops._corr_scratch, ops._call_scratch):
        for buf in d.values():
            buf.fill_(0xFF)


def hold_record(c, prec, reserve, rec, scratch_floats=P.SCRATCH_FLOATS):
    """The corr record against the restated planner; returns the launch and the occupancies that fit."""
    keys = ('kernel', 'workgroups', 'tiles', 'tiles_whole', 'streamk_units')
    got = {k: rec[k] for k in keys}
    plans = {occ: P.plan_corr(c, prec, occ, reserve, scratch_floats) for occ in P.OCCS}
    fits = {occ for occ, (_, want) in plans.items() if want == got}
    assert fits, (c.name, prec, reserve, 'record', got, 'planner', {o: p[1] for o, p in plans.items()})
    ln = plans[1][0]
    OCC[ln.key] = OCC.get(ln.key, set(P.OCCS)) & fits
    assert OCC[ln.key], (c.name, prec, reserve, got, 'no single occupancy explains the records of', ln.key)
    return ln, fits


def note_classes(c, prec, reserve, ln, rec):
    for k in P.classify(ln, rec):
        SEEN.setdefault((P.group(c, prec), k), (c.name, prec, reserve, {
            k2: rec[k2] for k2 in ('kernel', 'workgroups', 'tiles', 'tiles_whole', 'streamk_units')}))


def close(what, prec, got, want64):
    ref = want64.abs().max().item()
    e = (got.detach().double().cpu() - want64).abs().max().item() / (ref if ref > 0 else 1.0)
    print('{} {}: max_rel = {:.3g} (bar {:g})'.format(what, prec, e, BARS[prec]))
    assert got.shape == want64.shape and e <= BARS[prec], (what, prec, e)


def check(what, prec, exact, got, want64):
    if exact:
        same('{} {}'.format(what, prec), got, want64)
    else:
        close(what, prec, got, want64)


def corr_outputs(c, i):
    """(closure that runs the call and returns its outputs as a tuple, the fp64 references)."""
    if c.kind == 'conv_fwd':
        src, w, b = to_src(i.src), dev(i.w), dev(i.b)
        shapes = [(c.B, c.M, c.L // c.S)]
        fn = lambda: (ops.conv1d_fwd(src, w, b, c.S, roll=c.roll, pad_mode=c.mode, padL=c.padL),)
        refs = (i.ref,)
    elif c.kind == 'deconv_fwd':
        src, w, b = to_src(i.src), dev(i.w), dev(i.b)
        shapes = [(c.B, c.N, c.S * c.Ls)]
        fn = lambda: (ops.deconv1d_fwd(src, w, b, c.S),)
        refs = (i.ref,)
    elif c.kind == 'conv_dgrad':
        da, w = dev(i.da), dev(i.w)
        shapes = [(c.B, c.N, c.L)]
        fn = lambda: (ops.conv1d_dgrad(da, w, c.L, c.S, roll=c.roll, padL=c.padL),)
        refs = (i.ref,)
    else:
        dy, w = dev(i.dy), dev(i.w)
        shapes = [(c.B, c.M0, c.Ls), (c.B, c.M - c.M0, c.Ls)]
        fn = lambda: ops.deconv1d_dgrad(dy, w, c.S, c.M0, need0=c.need0)
        refs = (i.ref[:, :c.M0] if (c.M0 > 0 and c.need0) else None, i.ref[:, c.M0:])
    return fn, refs, shapes


def run_corr(c, prec, reserve, exact=True):
    i = P.inputs(c, exact)
    fn, refs, shapes = corr_outputs(c, i)
    with reserved(reserve), mode(prec):
        poison_scratch()
        for s in shapes:
            poison(*s)
        out1 = fn()
        rec1 = ops.last_corr_launch()
        poison_scratch()
        out2 = fn()
        rec2 = ops.last_corr_launch()
    what = '{}: {} reserve {}'.format(c.kind, c.name, reserve)
    for o1, o2, ref in zip(out1, out2, refs):
        if ref is None:
            assert o1 is None and o2 is None, what
            continue
        check(what, prec, exact, o1, ref)
        assert torch.equal(o1, o2), (what, prec, 'the second call gave other bits')
    assert rec1 == rec2, (what, prec, rec1, rec2)
    ln, _ = hold_record(c, prec, reserve, rec1)
    if exact:
        note_classes(c, prec, reserve, ln, rec1)
    return rec1


def run_wgrad(c, prec, reserve, exact=True):
    i = P.inputs(c, exact)
    lo, hi = to_src(i.lo), to_src(i.hi)
    args = (c.K, c.S, c.padL, c.mode)
    pre = dev(i.prefill)
    with reserved(reserve), mode(prec):
        dw = pre.clone()
        poison_scratch()
        ops.wgrad(lo, hi, dw, *args, roll=c.roll)
        rec = ops.last_wgrad_launch()
        once = dw.clone()
        poison_scratch()
        ops.wgrad(lo, hi, dw, *args, roll=c.roll)
        rec2 = ops.last_wgrad_launch()
        again = pre.clone()
        ops.wgrad(lo, hi, again, *args, roll=c.roll)
    what = 'wgrad: {} reserve {}'.format(c.name, reserve)
    w = P.launch_wgrad2(c)
    occ = rec['resident_per_cu']
    assert rec == rec2 and rec['kernel'] == 2 and 1 <= occ <= 4, (what, prec, rec, rec2)
    splits, cps = P.wgrad2_plan(w.tiles, w.nch, P.grid_slots(occ, reserve))
    assert (rec['tiles'], rec['splits'], rec['chunks_per_split']) == (w.tiles, splits, cps), (
        what, prec, rec, (w.tiles, splits, cps))
    p64 = i.prefill.double()
    check(what, 'fp32', exact, once, p64 + i.ref)
    check(what + ' twice', 'fp32', exact, dw, p64 + 2 * i.ref)
    if prec == 'det' or exact:
        assert torch.equal(once, again), (what, prec, 'a repeat from the same pre-fill gave other bits')
    if exact:
        WSEEN.setdefault(c.name, {})[reserve] = (occ, splits, cps, w.nch)


# ---------------------------------------------------------------------------------------------
# exact leg
# ---------------------------------------------------------------------------------------------
CORR_PARAMS = [(c, p, r) for c in P.CORR for p in P.precisions(c) for r in P.RESERVES]
WGRAD_PARAMS = [(c, p, r) for c in P.WGRAD for p in ('fp32', 'det') for r in P.RESERVES]


def _ids(params):
    return ['{}-{}-r{}'.format(c.name, p, r) for c, p, r in params]


@gpu
@pytest.mark.parametrize('c,prec,reserve', CORR_PARAMS, ids=_ids(CORR_PARAMS))
def test_corr_plan_exact(c, prec, reserve, reserve_guard):
    RAN.add((c.name, prec, reserve))
    run_corr(c, prec, reserve)


@gpu
@pytest.mark.parametrize('c,prec,reserve', WGRAD_PARAMS, ids=_ids(WGRAD_PARAMS))
def test_wgrad_plan_exact(c, prec, reserve, reserve_guard):
    RAN.add((c.name, prec, reserve))
    run_wgrad(c, prec, reserve)


# ---------------------------------------------------------------------------------------------
# random-valued leg: rounding paths under cut plans
# ---------------------------------------------------------------------------------------------
RANDOM = [(c, p, r) for c in P.CORR if c.rand for p in P.precisions(c) for r in (77, 512)] + \
         [(c, p, r) for c in P.WGRAD if c.rand for p in ('fp32', 'det') for r in (77, 512)]


@gpu
@pytest.mark.parametrize('c,prec,reserve', RANDOM, ids=_ids(RANDOM))
def test_random_valued_leg(c, prec, reserve, reserve_guard):
    (run_wgrad if c.kind == 'wgrad' else run_corr)(c, prec, reserve, exact=False)


# ---------------------------------------------------------------------------------------------
# scratch leg, straight through the C ABI
# ---------------------------------------------------------------------------------------------
SCRATCH_CASES = [next(c for c in P.CONV_FWD if c.name == 'p_f_pair_72'),
                 next(c for c in P.DECONV_FWD if c.name == 'p_t_72')]
SCRATCH_RESERVE = 77


def _abi_call(c, i, scratch_ptr, scratch_bytes):
    """One fp32 call of the case's entry point with the given scratch; (output, record)."""
    lib = _lib.load()
    src, w, b = to_src(i.src), dev(i.w), dev(i.b)
    cs = src.c_struct()
    pack = ops.WeightPack()
    if c.kind == 'conv_fwd':
        out = torch.full((c.B, c.M, c.L // c.S), float('nan'), device=DEV)
        rc = lib.segan_conv1d_fwd(ctypes.byref(cs), ops._ptr(pack.f(w, c.S)), ops._ptr(b), ops._ptr(out),
                                  c.B, c.N, c.M, c.L, c.K, c.S, c.padL, c.mode, c.roll, ops.PREC_FP32,
                                  scratch_ptr, scratch_bytes, ops._stream())
    else:
        pad = ops.deconv_pad(c.K, c.S)
        out = torch.full((c.B, c.N, c.S * c.Ls), float('nan'), device=DEV)
        rc = lib.segan_deconv1d_fwd(ctypes.byref(cs), ops._ptr(pack.t(w, c.S, pad)), None, ops._ptr(b),
                                    ops._ptr(out), c.B, c.M, c.N, c.Ls, c.K, c.S, pad, ops.ACT_NONE,
                                    ops.PREC_FP32, scratch_ptr, scratch_bytes, ops._stream())
    assert rc == 0, (c.name, rc, lib.segan_last_error().decode())
    return out, ops.last_corr_launch()


@gpu
@pytest.mark.parametrize('c', SCRATCH_CASES, ids=[c.name for c in SCRATCH_CASES])
def test_scratch_conditions_of_plan_streamk(c, reserve_guard):
    i = P.inputs(c, True)
    GUARD = 4096
    with reserved(SCRATCH_RESERVE):
        full_ptr, full_bytes = ops._scratch()
        poison_scratch()
        out, rec = _abi_call(c, i, full_ptr, full_bytes)
        same(c.name + ' full scratch', out, i.ref)
        ln, fits = hold_record(c, 'fp32', SCRATCH_RESERVE, rec)
        assert rec['streamk'] and rec['workgroups'] in {P.grid_slots(o, SCRATCH_RESERVE) for o in fits}, rec
        G = rec['workgroups']
        need = G * 2 * ln.slab                                # floats: G workgroups x 2 slabs of MB x NB
        classic = dict(kernel=rec['kernel'], workgroups=rec['tiles'], tiles=rec['tiles'],
                       tiles_whole=rec['tiles'], streamk_units=0)
        buf = torch.empty(need + GUARD, device=DEV, dtype=torch.float32)
        nan_bytes = buf.view(torch.uint8)
        for what, ptr, floats, want in (
                ('NULL', None, 0, classic),
                ('one float short', ctypes.c_void_p(buf.data_ptr()), need - 1, classic),
                ('exact size', ctypes.c_void_p(buf.data_ptr()), need, None)):
            nan_bytes.fill_(0xFF)
            out, r = _abi_call(c, i, ptr, floats * 4)
            same('{} scratch {}'.format(c.name, what), out, i.ref)
            got = {k: r[k] for k in classic}
            assert got == (want or {k: rec[k] for k in classic}), (c.name, what, r)
            hold_record(c, 'fp32', SCRATCH_RESERVE, r, scratch_floats=floats)
            # nothing behind the size that was passed is written (with NULL: nothing at all)
            tail = nan_bytes[4 * (floats if what == 'exact size' else 0):]
            assert bool((tail == 0xFF).all()), (c.name, what, 'bytes behind the scratch were written')
        # the exact-size run did use its slabs
        assert not bool((nan_bytes[:4 * need] == 0xFF).all()), c.name


# ---------------------------------------------------------------------------------------------
# closing: what this device executed, and the reserve
# ---------------------------------------------------------------------------------------------
@gpu
def test_every_plan_class_was_executed(reserve_guard):
    expect = {(c.name, p, r) for c, p, r in CORR_PARAMS + WGRAD_PARAMS}
    if RAN != expect:
        # a partial selection (-k, one test id); a case that was started and failed is in RAN, and
        # the classes it alone would have reached are then reported missing below
        pytest.skip('only {} of the {} exact-leg tests were selected in this session'.format(
            len(RAN), len(expect)))
    for (g, k), (name, prec, reserve, rec) in sorted(SEEN.items(), key=lambda kv: (str(kv[0][0]), kv[0][1])):
        print('{:7s} {:4} {:46s} {:16s} {:6s} reserve {:3d}  wg {:4d} tiles {:4d} whole {:4d} units {:2d}'.format(
            g, k, P.CLASS_NAMES[k], name, prec, reserve, rec['workgroups'], rec['tiles'],
            rec['tiles_whole'], rec['streamk_units']))
    for key, occ in sorted(OCC.items(), key=str):
        print('occupancy', sorted(occ), 'of', key)
    for name, by_reserve in sorted(WSEEN.items()):
        print('wgrad', name, {r: v for r, v in sorted(by_reserve.items())}, '(occ, splits, chunks per split, chunks)')
    assert not P.missing(SEEN), 'classes not executed on this device: {}'.format(P.missing(SEEN))
    assert any(len({v[1] for v in by.values()}) >= 3 for by in WSEEN.values()), WSEEN
    assert any(v[1] > 1 and v[3] % v[2] for by in WSEEN.values() for v in by.values()), WSEEN


@gpu
def test_reserve_is_back_where_it_started(reserve_guard):
    now = ops.set_reserved_slots(0)
    ops.set_reserved_slots(now)
    assert now == reserve_guard == STATE['start']
