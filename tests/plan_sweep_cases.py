"""TEST-ONLY host side of tests/test_gpu_plan_sweep.py: the case table, the reserves, the launch
planners restated as pure functions, and the classes of launch plan the sweep must execute.  Nothing
here touches a GPU.  The input builders, the fp64 references and the exactness condition are those
of tests/src_sweep_cases.py (imported, and its constructors F / D / G / X / W build the cases).

Every forward / data-gradient contraction and the fp32 weight gradient plan their launch from
``G = segan_grid_slots(occ)``: 256 x resident workgroups per CU (at most 4), minus the reserve
(segan_set_reserved_slots, clamped to [0, 512]), floored at 64.  Every case of the table runs under
every reserve of RESERVES, which gives these grids:

    reserve      0      5     77    509    512
    occ 1      256    251    179     64     64
    occ 2      512    507    435     64     64
    occ 3      768    763    691    259    256
    occ 4     1024   1019    947    515    512

5, 77 and 509 are no multiples of 8; 509 is there because 5 and 77 leave occupancy 4 with more than
900 workgroups, and a stream-K launch with whole tiles AND an odd grid then needs more than 1000
tiles.  The clamp at 512 means that no reserve brings occupancy 4 below 512 workgroups: 512 is the
value that comes closest to "64 .. 256 for every occupancy" (64, 64, 256, 512).

``plan_streamk`` (segan_conv.hip), the rule of ``launch_bf2`` (segan_conv_bf2.hip) and
``wgrad2_plan`` (segan_wgrad.hip) are restated below as functions of (tiles, chunks, G, ...); the
tile geometry comes from ``launch_fp32`` / ``launch_bf2`` / ``launch_wgrad2``, which follow
launch_corr_f / launch_corr_tt / segan_corr_bf2_* / launch_wgrad2 and take the kernel from
src_sweep_cases.plan_corr_f / plan_corr_t / plan.
"""
import types

import src_sweep_cases as T

REFLECT, ZERO = T.REFLECT, T.ZERO
RESERVES = (0, 5, 77, 509, 512)
OCCS = (1, 2, 3, 4)
SCRATCH_FLOATS = 1024 * 2 * 128 * 128          # segan_corr_scratch_bytes() / 4: what ops passes


def ns(**kw):
    return types.SimpleNamespace(**kw)


def cdiv(a, b):
    return -(-a // b)


def grid_slots(occ, reserve):
    """segan_grid_slots under segan_set_reserved_slots(reserve)."""
    return max(64, 256 * occ - min(max(reserve, 0), 512))


# ---------------------------------------------------------------------------------------------
# the table.  Tiles are 128 columns of B * (row length) positions; "tiles" in the comments is what
# the fp32 launcher counts.  Stream-K needs >= 64 tiles, >= 8 chunks, and a last round of 256 that
# is less than 97 % full; the persistent grid needs >= 512 * occ tiles
# ---------------------------------------------------------------------------------------------
N_ = None
CONV_FWD = [
    # corr2_kernel, paired channels (K = 31, N even): 72 tiles of 8 chunks, one row tile
    T.F('p_f_pair_72', 3, (8, 0), '', 66, 4 * 3072, 4, N_, roll=5),
    # corr2_kernel, 9 chunks (no pairs; pieces of 2, 4, 5 chunks span two tiles), zero padding
    T.F('p_f_odd_100', 2, (4, 5), 'cl', 70, 4 * 6400, 4, N_, mode=ZERO, padL=15, rand=True),
    # corr_kernel (a shift under zero padding): 80 tiles of 11 chunks, a ragged last tile per sample
    T.F('p_f_k1_80', 2, (5, 6), 'hl', 65, 4 * 5100, 4, N_, mode=ZERO, padL=7, roll=-3, rand=True),
    # 16 channels, two row tiles: the bf16 kernel cuts it too (8 stages of 8 channels)
    T.F('p_f_bf_80', 2, (7, 9), 'c', 130, 4 * 2560, 4, N_, roll=-2, rand=True),
    # stride 2: 16 phases per channel
    T.F('p_f_s2_72', 2, (8, 0), 'l', 80, 2 * 4608, 2, N_, roll=1),
    # 600 tiles: whole rounds AND a cut remainder under every grid of the table
    T.F('p_f_600', 2, (8, 0), '', 65, 4 * 38400, 4, N_, roll=-1),
    # 2051 tiles of 3 chunks: the persistent grid, a partial last round (2051 is prime)
    T.F('p_f_persist', 1, (3, 0), '', 65, 4 * 128 * 2051, 4, N_, K=5, roll=2),
    # 30 tiles: classic whatever the grid
    T.F('p_f_classic', 2, (8, 0), 'h', 66, 4 * 1920, 4, N_),
]

DECONV_DGRAD = [
    # the first row tile (128 rows of dx0 = NULL) is dead and left out: 72 live tiles, paired
    T.X('p_x_dead_72', 2, 192, 128, 8, 4608, 4, N_, need0=False, rand=True),
    # dx0 = NULL ends inside the first row tile: 2 x 36 tiles, all live, rows below 100 unstored
    T.X('p_x_partdead_72', 2, 160, 100, 9, 2304, 4, N_, need0=False),
    # both destinations, split inside the first row tile
    T.X('p_x_on_80', 2, 130, 64, 10, 2560, 4, N_, need0=True),
]

DECONV_FWD = [
    # corr2_kernel: 72 tiles of 8 chunks (32 channels x 8 taps)
    T.D('p_t_72', 3, (16, 16), 'cl', 5, 3072, 4, N_, rand=True),
    # corr_kernel (a shift): 2 row tiles x 50, 10 chunks
    T.D('p_t_k1_100', 2, (20, 20), 'hl', 33, 3200, 4, N_, rand=True),
    # 600 tiles of 16 chunks; 64 channels: bf16 cuts it (8 stages)
    T.D('p_t_600', 2, (64, 0), '', 3, 38400, 4, N_),
    # 2051 tiles of one chunk: the persistent grid
    T.D('p_t_persist', 1, (4, 0), '', 3, 128 * 2051, 4, N_),
    # stride 2 (16 taps per channel): 80 tiles of 8 chunks
    T.D('p_t_s2_80', 2, (16, 0), 'c', 40, 5120, 2, N_),
    T.D('p_t_classic', 2, (32, 0), '', 4, 1920, 4, N_),
]

CONV_DGRAD = [
    # the padded row is 5127 columns: 81 tiles, samples change inside a tile; 8 chunks, folded halo
    T.G('p_g_81', 2, 12, 32, 4 * 5120, 4, N_, roll=-7, rand=True),
    T.G('p_g_600', 1, 3, 64, 4 * 76700, 4, N_, roll=3),
]

PLAIN = T.PLAIN
WGRAD = [
    # 2 tiles, 88 chunks of 32 columns: three or more split counts over RESERVES at every occupancy
    T.W('p_w_2tiles', 2, ((40, 0), PLAIN), ((6, 0), PLAIN), 1408, 4, N_, roll=3),
    # 6 tiles, 72 chunks; a materialised lo and a transformed hi; zero padding
    T.W('p_w_6tiles', 3, ((120, 10), 'cl'), ((5, 7), 'cl'), 768, 4, N_, mode=ZERO, rand=True),
    # stride 2, a 64-row tile: 3 tiles, 100 chunks
    T.W('p_w_s2', 2, ((48, 0), PLAIN), ((10, 0), 'hl'), 1600, 2, N_, roll=-1),
]

TABLES = {'conv_fwd': CONV_FWD, 'deconv_fwd': DECONV_FWD, 'conv_dgrad': CONV_DGRAD,
          'deconv_dgrad': DECONV_DGRAD, 'wgrad': WGRAD}
CORR = CONV_FWD + DECONV_DGRAD + DECONV_FWD + CONV_DGRAD
ALL = CORR + WGRAD
# the inputs of a case are seeded by (kind, name): keep the names apart from the src sweep's
for _kind, _cases in TABLES.items():
    assert not {c.name for c in _cases} & {c.name for c in T.TABLES[_kind]}
inputs, check_exact = T.inputs, T.check_exact


def form(c):
    return 'F' if c.kind in ('conv_fwd', 'deconv_dgrad') else 'T'


# ---------------------------------------------------------------------------------------------
# tile geometry of a launch (launch_corr_f / launch_corr_tt, segan_corr_bf2_f / _t, launch_wgrad2)
# ---------------------------------------------------------------------------------------------
def _args(c):
    """The CorrArgs fields the launchers read, as the four entry points of segan_conv.hip set them."""
    S, U = c.S, 32 // c.S
    a = ns(U=U, S=S, B=c.B, xfm=0, C0=0, C1=0, zero=True, pair=False, rows=0, Nout=0, rt0_rows=0,
           shift=False, halo=False)
    if c.kind == 'conv_fwd':
        a.rows, a.Tcols, a.Ktot, a.Cv, a.H = c.M, c.L // S, c.N * 32, c.N * S, U - 1
        a.xfm, (a.C0, a.C1), a.zero = T.xf_mode(c.xf), c.seg, c.mode == ZERO
        a.pair = c.K == 31 and c.N > 2 and c.N % 2 == 0
    elif c.kind == 'deconv_dgrad':
        a.rows, a.Tcols, a.Ktot, a.Cv, a.H = c.M, c.Ls, c.N * 32, c.N * S, U - 1
        a.C0 = c.N
        a.pair = c.K == 31 and c.N > 2 and c.N % 2 == 0
        a.rt0_rows = c.M0 if (c.M0 > 0 and not c.need0) else 0      # rows of a NULL out0
    elif c.kind == 'deconv_fwd':
        sh = T._t_shifts(c.K, S)
        a.Nout, a.Tcols, a.Ktot, a.Cv, a.H = c.N, c.Ls, c.M * U, c.M, U - 1 + max(sh)
        a.xfm, (a.C0, a.C1), a.shift = T.xf_mode(c.xf), c.seg, any(sh)
        a.mask = sum(1 << r for r, s in enumerate(sh) if s)
    elif c.kind == 'conv_dgrad':
        padR = max(c.K - S - c.padL, 0)
        a.Nout, a.Tcols, a.Ktot, a.Cv, a.H = c.N, (c.L + c.padL + padR - 1) // S + 1, c.M * U, c.M, U - 1
        a.C0, a.halo, a.mask = c.M, True, 0
    else:
        raise ValueError(c.kind)
    a.Ctot = c.B * a.Tcols
    return a


def launch_fp32(c, blocked=False):
    """The fp32 launch of a corr case (`blocked`: under ops.set_accumulation('blocked')): kernel id, tile (MB x NB), chunk length KC, tiles, chunks,
    whether stream-K and the persistent grid are allowed, paired cuts, and `key`, which names the
    kernel instance and its LDS size — what the occupancy depends on."""
    a = _args(c)
    U, S = a.U, a.S
    NB = 128
    spt = T.samples_per_tile(a.Tcols, NB)
    RLs = NB + spt * a.H
    if form(c) == 'F':
        assert not (U == 16 and a.rows <= 32), 'the 32 x 256 tile of launch_corr_f is not restated'
        kern = T.plan_corr_f(U, a.rows, a.Tcols, a.zero, a.xfm, a.C0, a.C1)
        small = a.rows <= 64
        MB, allow = (64, False) if small else (128, True)
        if kern == 2:
            KC = 32
        else:
            KC = 32 if (RLs <= 256 and not small and U <= 16) else 64
        nrow = cdiv(a.rows, MB)
        rt0 = a.rt0_rows // MB
    else:
        kern = T.plan_corr_t(U, a.H, a.Tcols, a.xfm, a.C0, a.C1)
        MB, allow, rt0 = 128, True, 0
        if kern == 2:
            KC = 32
            if U == 16:
                narrow = not a.shift and a.Nout <= 16
                if a.Nout <= 32 and (not a.halo or a.Nout <= 16) and T._corr2_ok(
                        U, a.H, a.Tcols, 256, True, a.xfm, a.C0, a.C1):
                    NB = 256
                    RLs = NB + T.samples_per_tile(a.Tcols, NB) * a.H
                    MB = 32 if narrow else 64
                elif narrow:
                    MB = 32
                elif a.Nout <= 32:
                    MB = 64
            nrow = cdiv(a.Nout, MB // S)
        else:
            KC = 32 if (RLs <= 256 and U <= 16) else 64
            nrow = cdiv(a.Nout, 128 // S)                  # NP / (MB / S)
    if kern == 2:
        RLs = cdiv(RLs, 64 * (4 // (32 // U))) * 64 * (4 // (32 // U))
    ntiles = (nrow - rt0) * cdiv(a.Ctot, NB)
    return ns(kernel=kern, MB=MB, NB=NB, KC=KC, ntiles=ntiles, nch=cdiv(a.Ktot, KC), allow=allow,
              pair_cuts=kern == 2 and a.pair, rt0=rt0, dead=a.rt0_rows > 0, slab=MB * NB,
              key=('blocked' if blocked and blocked_variant(kern, U, MB) else 'fp32', kern, form(c), U, MB,
                   NB, KC, a.shift, a.xfm != 0, RLs))


def blocked_variant(kern, U, MB):
    """launch_corr2_t: blocked accumulation is built for corr2_kernel's stride-4 128-row tiles."""
    return kern == 2 and U == 8 and MB == 128


def bf2_takes(c, prec):
    """Does this case run corr_bf2_kernel in `prec` ('bf16' / 'bf16x3')?"""
    return T.plan(c, prec) == 3


def launch_bf2(c, prec):
    """The bf16 / bf16x3 launch (launch_bf2): 128 x 128 tiles; a tile is `nst` weight stages."""
    a = _args(c)
    U, S = a.U, a.S
    TCH = U if prec == 'bf16x3' else U // (4 if U >= 8 else U)
    nrow = cdiv(a.rows, 128) if form(c) == 'F' else cdiv(a.Nout, 128 // S)
    rt0 = a.rt0_rows // 128
    RLs = cdiv(128 + T.samples_per_tile(a.Tcols, 128) * a.H, 64) * 64
    return ns(kernel=3, ntiles=(nrow - rt0) * cdiv(a.Ctot, 128), nch=cdiv(a.Cv, 16) * TCH, rt0=rt0,
              dead=a.rt0_rows > 0, pair_cuts=False, slab=128 * 128,
              key=(prec, 3, form(c), U, getattr(a, 'mask', 0), RLs))


def launch_wgrad2(c):
    """wgrad2_kernel's tiles and chunks (wgrad2_plan's first lines, launch_wgrad2_rows)."""
    assert T.plan(c, 'fp32') == 2, c.name
    U = 32 // c.S
    MB = (32 if c.M <= 32 else 64 if c.M <= 64 else 128) if U == 16 else 128
    return ns(tiles=cdiv(c.N * c.S, 128 // U) * cdiv(c.M, MB), nch=cdiv(c.B * c.Ls, 32))


# ---------------------------------------------------------------------------------------------
# the planners
# ---------------------------------------------------------------------------------------------
def _record(workgroups, tiles, whole, units):
    """What segan_debug_last_corr reports (ops.last_corr_launch), less kernel id and xf_mode."""
    return dict(workgroups=workgroups, tiles=tiles, tiles_whole=whole, streamk_units=units)


def plan_streamk(ntiles, nch, G, occ, allow=True, pair_cuts=False, scratch_floats=SCRATCH_FLOATS,
                 slab_floats=128 * 128):
    """plan_streamk of segan_conv.hip (activation NONE)."""
    classic_eff = ntiles / (256.0 * cdiv(ntiles, 256))
    if not allow or ntiles < 64 or nch < 8 or classic_eff >= 0.97:
        if allow and ntiles >= 2 * 256 * occ:
            return _record(G, ntiles, ntiles, 0)           # persistent, whole tiles
        return _record(ntiles, ntiles, ntiles, 0)
    if scratch_floats < G * 2 * slab_floats:
        return _record(ntiles, ntiles, ntiles, 0)
    whole = (ntiles // G) * G
    rem = ntiles - whole
    if rem == 0:
        return _record(ntiles, ntiles, ntiles, 0)
    units = cdiv(rem * nch, G)
    if pair_cuts:
        units += units & 1
    return _record(G, ntiles, whole, units)


def plan_bf2(ntiles, nst, G, scratch_floats=SCRATCH_FLOATS):
    """The stream-K rule of launch_bf2 (segan_conv_bf2.hip): no persistent grid of whole tiles."""
    classic_eff = ntiles / (256.0 * cdiv(ntiles, 256))
    if ntiles >= 64 and nst >= 8 and classic_eff < 0.97:
        rem = ntiles % G
        if rem > 0 and scratch_floats >= G * 2 * 128 * 128:
            return _record(G, ntiles, ntiles - rem, cdiv(rem * nst, G))
    return _record(ntiles, ntiles, ntiles, 0)


def wgrad2_plan(tiles, nch, G):
    """wgrad2_plan of segan_wgrad.hip: (splits, chunks per split)."""
    best, best_eff = 1, 0.0
    ns_max = max(nch // 8, 1)
    n = 1
    while n <= ns_max and tiles * n <= 4 * G:
        blocks = tiles * n
        eff = blocks / (float(G) * cdiv(blocks, G))
        if eff > best_eff + 0.02:
            best_eff, best = eff, n
        n += 1
    cps = cdiv(nch, best)
    return cdiv(nch, cps), cps


FP32_ONLY = ('p_f_persist', 'p_t_persist')     # 2051 tiles: the persistent grid is an fp32 plan


def precisions(c):
    """The precisions a corr case runs in: fp32, and the bf16 modes whose kernel takes it."""
    if c.name in FP32_ONLY:
        return ['fp32']
    ln = launch_fp32(c)
    blocked = ['blocked'] if blocked_variant(ln.kernel, 32 // c.S, ln.MB) else []
    return ['fp32'] + blocked + [p for p in ('bf16x3', 'bf16') if bf2_takes(c, p)]


def plan_corr(c, prec, occ, reserve, scratch_floats=SCRATCH_FLOATS):
    """(launch, record) of a corr case in `prec` at occupancy `occ` under `reserve`."""
    G = grid_slots(occ, reserve)
    if prec in ('fp32', 'blocked'):
        ln = launch_fp32(c, prec == 'blocked')
        rec = plan_streamk(ln.ntiles, ln.nch, G, occ, ln.allow, ln.pair_cuts, scratch_floats, ln.slab)
    else:
        ln = launch_bf2(c, prec)
        rec = plan_bf2(ln.ntiles, ln.nch, G, scratch_floats)
    rec['kernel'] = ln.kernel
    return ln, rec


# ---------------------------------------------------------------------------------------------
# classes
# ---------------------------------------------------------------------------------------------
def spans_two_tiles(nch, units, total):
    """Does a stream-K piece (units [g units, (g + 1) units) below total) hold chunks of two tiles?"""
    return any(u0 // nch != (min(u0 + units, total) - 1) // nch for u0 in range(0, total, units))


def classify(ln, rec):
    """The classes (module docstring of test_gpu_plan_sweep.py) a corr launch record belongs to."""
    wg, tiles, whole, units = (rec[k] for k in ('workgroups', 'tiles', 'tiles_whole', 'streamk_units'))
    out = set()
    if units == 0:
        if wg == tiles:
            out.add(1)
        elif wg < tiles and tiles % wg:
            out.add(2)
            if wg % 8:
                out.add(8.2)
        return out
    out.add(3 if whole == 0 else 4)
    if whole and wg % 8:
        out.add(8.4)
    if spans_two_tiles(ln.nch, units, (tiles - whole) * ln.nch):
        out.add(5)
    if ln.pair_cuts:
        out.add(6)
        if cdiv((tiles - whole) * ln.nch, wg) & 1:
            out.add(6.1)                                   # the cut was moved to an even chunk
    if ln.dead:
        out.add(7)
    return out


FP32_CLASSES = (1, 2, 3, 4, 5, 7, 8.2, 8.4)               # per form; 6 and 6.1 on the F form only
BF_CLASSES = (3, 4, 5)
CLASS_NAMES = {1: 'classic', 2: 'persistent grid, partial last round', 3: 'stream-K, no whole tiles',
               4: 'stream-K behind whole tiles', 5: 'a piece spanning two tiles', 6: 'paired channels',
               6.1: 'paired channels, cut moved to an even chunk', 7: 'beside dead tiles',
               8.2: 'persistent grid no multiple of 8', 8.4: 'stream-K grid no multiple of 8, whole tiles'}


def wanted():
    """Every (group, class) the sweep must execute: group 'F' / 'T' (fp32), 'bf16', 'bf16x3', and
    'blocked' (corr2_kernel's blocked-accumulation instances, either form)."""
    want = {(f, k) for f in 'FT' for k in FP32_CLASSES if not (f == 'T' and k == 7)}
    want |= {('F', 6), ('F', 6.1)}
    want |= {(p, k) for p in ('bf16', 'bf16x3') for k in BF_CLASSES}
    want |= {('blocked', k) for k in BF_CLASSES + (6.1,)}
    return want


def group(c, prec):
    return form(c) if prec == 'fp32' else prec


def missing(seen):
    return sorted('{}: {}'.format(g, CLASS_NAMES[k]) for g, k in wanted() - set(seen))
