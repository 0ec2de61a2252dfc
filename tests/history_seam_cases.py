"""Shared by tests/test_history_seams_cpu.py and tests/test_history_seams_gpu.py: the inputs that take k_history_record /
k_history_seed (and, past 512 rows, k_phase_apply / k_phase_seed and k_surface_loss) to the places where the flags summary, the
load form, the comparisons and the device clock could be wrong without tests/test_history_gpu.py noticing -- grids whose
16 x 16 x 16 bricks are partly all-solid, a box whose summary has a second word per (j, k) brick row, directed (A, B) pairs on
every comparison of the recorder, births that cross the planes 15 | 16 and 31 | 32, and a run of 401 steps through the graph.

Nothing here is stored and nothing is computed on a device: every expected value comes from ThermalHistory.record_reference /
seed_reference, PhaseChange.correct and the pinned C oracle.  The classes of the device module are passed in, so this module
imports neither the device module nor torch."""
import math

import numpy as np

import history_cases as hc
import seam_cases as sc
from history_cases import CP, FACES, K, KAPPA, RHO  # noqa: F401
from seam_cases import BOXES, DX, MARKER, TINF  # noqa: F401

BRICK = 16
MARKS = (MARKER, MARKER + 1.0, MARKER + 2.0)      # what the off-mask cells of T_peak, t_hi, t_lo hold before a record launch
LEVELS = (800.0, 500.0, 1400.0)


def up(x):
    return float(np.nextafter(x, np.inf))


def dn(x):
    return float(np.nextafter(x, -np.inf))


# ---- the flags summary, predicted from the mask -------------------------------------------------------------------------------
def embed(a, phys, fill=False):
    out = np.full(phys, fill, dtype=np.asarray(a).dtype)
    out[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return out


def predicted_bricks(mask, phys):
    """(nbx, nby, nbz) bool: the bit of a brick is set exactly when every cell of the brick inside the physical box `phys`, and
    every neighbour of such a cell inside that box, is in the mask (the cells of the physical box outside the logical one are
    off the mask)"""
    m = embed(np.asarray(mask, dtype=bool), phys)
    p = np.pad(m, 1, constant_values=True)                       # a neighbour outside the box does not count
    ok = m.copy()
    for a in range(3):
        for d in (-1, 1):
            sl = tuple(slice(1 + (d if i == a else 0), 1 + (d if i == a else 0) + m.shape[i]) for i in range(3))
            ok &= p[sl]
    nb = [(n + BRICK - 1) // BRICK for n in phys]
    out = np.zeros(nb, dtype=bool)
    for bi in range(nb[0]):
        for bj in range(nb[1]):
            for bk in range(nb[2]):
                out[bi, bj, bk] = ok[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16, 16 * bk:16 * bk + 16].all()
    return out


def summary_word(bi, bj, bk, phys):
    """(index of the 32-bit word, bit) of brick (bi, bj, bk) in the flags summary of the physical box `phys`"""
    nbx, nbz = (phys[0] + BRICK - 1) // BRICK, (phys[2] + BRICK - 1) // BRICK
    bwx = (nbx + 31) // 32
    return (bj * nbz + bk) * bwx + bi // 32, bi % 32


def summary_bits(words, phys):
    """the downloaded summary (uint32 words) -> (nbx, nby, nbz) bool"""
    w = np.asarray(words).view(np.uint32)
    nb = [(n + BRICK - 1) // BRICK for n in phys]
    out = np.zeros(nb, dtype=bool)
    for bi in range(nb[0]):
        for bj in range(nb[1]):
            for bk in range(nb[2]):
                i, b = summary_word(bi, bj, bk, phys)
                out[bi, bj, bk] = bool((int(w[i]) >> b) & 1)
    return out


def vector_form(pd, flags_ptr, *field_ptrs):
    """the rule of adi_history_record / adi_history_seed, restated: pairs of cells are loaded with one 16-byte (fields) and one
    2-byte (flags) instruction when rows and planes have even strides, the flags start on an even address and every field that
    is loaded in pairs starts on a 16-byte boundary"""
    return pd[2] % 2 == 0 and pd[3] % 2 == 0 and flags_ptr % 2 == 0 and all(p % 16 == 0 for p in field_ptrs)


def pool_bricks(pool):
    """per axis: the bricks of the smallest and the largest index of the pool"""
    return [(int(pool['lo'][a]) // BRICK, int(pool['hi'][a]) // BRICK) for a in range(3)]


def spans_two_bricks(pool, shape):
    return pool['cells'] > 0 and all(n <= BRICK or lo < hi for n, (lo, hi) in zip(shape, pool_bricks(pool)))


def definition_steps(TH, levels, mask, fields, t, dt):
    """seed from fields[0], then the steps fields[n] -> fields[n + 1] as single recorded steps -> (states, pools, times)"""
    state = TH.seed_reference(hc.empty_state(mask.shape), fields[0], mask)
    states, pools, times = [state], [], []
    for A, B in zip(fields, fields[1:]):
        state, pool = TH.record_reference(state, A, B, mask, t, dt, levels)
        t = t + dt
        states.append(state)
        pools.append(pool)
        times.append(t)
    return states, pools, times


# ---- 1. mixed bricks, both load forms -----------------------------------------------------------------------------------------
MIXED = ('S1', 'S1p', 'S2', 'S3')
MIXED_SCALE = (1.15, 0.95, 0.5, 1.2)               # fields[n] = scale * seam_cases.field_of(shape, seed 7 + n)
MIXED_DT, MIXED_T0 = 0.25, 2.0


def mixed_fields(name):
    """four fields: hot, a little cooler (the pool shrinks), cold (no pool, most cells cross T_hi or both levels), hot again"""
    shape = BOXES[name][0]
    return [s * sc.field_of(shape, seed=7 + n) for n, s in enumerate(MIXED_SCALE)]


def seam_sel(shape):
    """single cells on the planes 15, 16, 31, 32 of axis 2 (those the box has), on both sides of i = 16 and of j = 16"""
    sel = np.zeros(shape, dtype=bool)
    for k in (15, 16, 31, 32):
        if k < shape[2]:
            for i, j in ((15, 2), (15, 8), (16, 5), (16, 11), (2, 15), (8, 15), (5, 16), (11, 16), (15, 15), (16, 16)):
                sel[i, j, k] = True
    return sel


# ---- 2. rows past 512 -----------------------------------------------------------------------------------------------------------
LONG_SHAPE = (560, 48, 48)
LONG_HOLE = (535, 24, 24)                          # in brick (33, 1, 1)
LONG_CAVITY = (534, 537, 23, 26, 23, 26)           # 3 x 3 x 3, wholly inside brick (33, 1, 1)
LONG_FAR, LONG_NEAR = (33, 1, 1), (1, 1, 1)        # the brick with the hole (second summary word) and its untouched counterpart
LONG_LAW = (2.7e5, 1400.0, 1450.0)
LONG_DT, LONG_T0 = 0.25, 3.0


def long_mask(cavity):
    m = np.ones(LONG_SHAPE, dtype=bool)
    if cavity:
        i0, i1, j0, j1, k0, k1 = LONG_CAVITY
        m[i0:i1, j0:j1, k0:k1] = False
    else:
        m[LONG_HOLE] = False
    return m


def _long_hot():
    hot = np.zeros(LONG_SHAPE, dtype=bool)
    hot[10:40, 10:40, 10:40] = True
    hot[520:550, 10:40, 10:40] = True
    return hot


_long = {}


def long_fields():
    """three fields: 1700 degrees over bricks (1, 1, 1) and (33, 1, 1) and a margin around them in a cold body; a little cooler
    (still a pool in both bricks); then a field between 400 and 900 degrees there: crossings of one level and of both"""
    if 'f' not in _long:
        rng = np.random.default_rng(560)
        hot = _long_hot()
        x = (np.arange(LONG_SHAPE[0]) % 16 / 16.0)[:, None, None]
        A = np.where(hot, 1700.0, 300.0) + rng.uniform(-20.0, 20.0, LONG_SHAPE)
        B1 = np.where(hot, 1560.0, 290.0) + rng.uniform(-20.0, 20.0, LONG_SHAPE)
        B2 = np.where(hot, 400.0 + 500.0 * x, 280.0) + rng.uniform(-20.0, 20.0, LONG_SHAPE)
        for a in (A, B1, B2):
            a.setflags(write=False)
        _long['f'] = [A, B1, B2]
    return _long['f']


def long_melt_field():
    """the start of the latent-heat step: above the liquidus over both bricks, solid elsewhere"""
    return np.where(_long_hot(), 1700.0, 900.0)


def brick_cells(b, shape):
    out = np.zeros(shape, dtype=bool)
    out[16 * b[0]:16 * b[0] + 16, 16 * b[1]:16 * b[1] + 16, 16 * b[2]:16 * b[2] + 16] = True
    return out


# ---- 3. every comparison at its edge --------------------------------------------------------------------------------------------
EDGE_SHAPE = (16, 16, 32)                          # bricks (0, 0, 0) and (0, 0, 1)
EDGE_LEVELS = {'usual': LEVELS, 'zero': (0.0, -5.0, 0.0)}
EDGE_DT, EDGE_T0 = 0.5, 1.25


def edge_table(levels):
    """the directed (A, B) pairs, A the seed (so T_peak = A before the step)"""
    hi, lo, melt = levels
    far, cold, mid, hot = hi + 700.0, lo - 200.0, 0.5 * (hi + lo), hi + 300.0
    three = lambda x: (dn(x), x, up(x))
    t = []
    for lev in (hi, lo):
        for a in three(lev):                       # A below, on and above the level; B below it, and on it
            t += [(a, cold), (a, dn(lev)), (a, lev)]
        for b in three(lev):                       # B below, on and above the level; A above it, and a hair above it
            t += [(hot, b), (up(lev), b)]
    for a in (cold, mid, hot, melt):               # B below, on and above the old peak
        t += [(a, dn(a)), (a, a), (a, up(a))]
    for b in three(melt):                          # B below, on and above T_melt, reached from below and from above
        t += [(cold, b), (far + 100.0, b)]
    t += [(up(hi), hi)]                            # the smallest denominator: the fraction is exactly 1
    t += [(hot, lo), (hot, cold), (up(hi), dn(lo))]                  # both crossings in one step
    t += [(np.inf, cold), (np.inf, mid), (np.inf, hot)]              # A = +inf: the fraction is inf / inf
    t += [(hot, np.nan), (cold, np.nan), (np.nan, cold), (np.nan, hot), (np.nan, np.nan)]
    t += [(1.0, -0.0), (1.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (-1.0, -0.0)]   # zeros of both signs
    if len(t) % 2 == 0:                            # an odd length: tiled over rows of 16, a pair meets even and odd k
        t += [(mid, cold)]
    return np.array(t, dtype=np.float64)


def edge_fields(which):
    """(A, B) over the 16 x 16 x 32 box: the table tiled over each brick, shifted by one entry in the second, so that every pair
    falls on even and odd k in both (the table's length is odd)"""
    t = edge_table(EDGE_LEVELS[which])
    assert len(t) % 2 == 1
    A, B = np.empty(EDGE_SHAPE), np.empty(EDGE_SHAPE)
    for b, shift in ((0, 0), (1, 1)):
        A[:, :, 16 * b:16 * b + 16] = sc.tile(t[:, 0], (16, 16, 16), shift)
        B[:, :, 16 * b:16 * b + 16] = sc.tile(t[:, 1], (16, 16, 16), shift)
    return A, B


def edge_classes(A, B, levels):
    """name -> bool array: the classes of cell the table is there for, from the fields alone"""
    hi, lo, melt = levels
    with np.errstate(invalid='ignore'):
        c = {}
        for nm, lev in (('hi', hi), ('lo', lo)):
            c['A_below_' + nm], c['A_on_' + nm], c['A_above_' + nm] = A == dn(lev), A == lev, A == up(lev)
            c['B_below_' + nm] = (B == dn(lev)) & (A > lev)
            c['B_on_' + nm] = (B == lev) & (A > lev)
            c['B_above_' + nm] = (B == up(lev)) & (A > lev)
        fin = np.isfinite(A)
        c['B_below_peak'], c['B_on_peak'], c['B_above_peak'] = fin & (B < A) & (B == np.nextafter(A, -np.inf)), fin & (B == A), \
            fin & (B == np.nextafter(A, np.inf))
        c['B_below_melt'], c['B_on_melt'], c['B_above_melt'] = B == dn(melt), B == melt, B == up(melt)
        c['fraction_one'] = (A == up(hi)) & (B == hi)
        c['both_crossings'] = (A > hi) & (B <= lo)
        c['A_inf'] = np.isposinf(A) & np.isfinite(B)
        c['B_nan'] = np.isnan(B) & ~np.isnan(A)
        c['A_nan'] = np.isnan(A)
        c['B_neg_zero'] = (B == 0.0) & np.signbit(B)
        c['A_neg_zero'] = (A == 0.0) & np.signbit(A)
    return c


VOTE_CELL = (3, 4, 16 + 5)


def vote_fields(bump):
    """brick 0 entirely at T_lo, brick 1 too but for one cell a hair above (bump); everything cools to 300"""
    lo = LEVELS[1]
    A, B = np.full(EDGE_SHAPE, lo), np.full(EDGE_SHAPE, 300.0)
    if bump:
        A[VOTE_CELL] = up(lo)
    return A, B


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(got, want):
    """NaN in the same places, and the same bit patterns everywhere else (so -0.0 is not 0.0; the sign and payload of a NaN
    are no part of the contract: inf / inf has them as the processor pleases)"""
    got, want = np.asarray(got), np.asarray(want)
    n = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), n) and np.array_equal(bits(got)[~n], bits(want)[~n])


# ---- 5. births across the seams -------------------------------------------------------------------------------------------------
BIRTH = dict(box='S1p', first=14, cross=(14, 18), planes_per_layer=2, Ts=1500.0, h=3000.0, theta=0.5, cfl=2.0,
             levels=(1450.0, 1395.0, 1440.0))


def birth_layers():
    """[(k0, k1)): the plate [0, 14), the layer across plane 15 | 16, then layers of two planes to the top of the box"""
    nz = BOXES[BIRTH['box']][0][2]
    k = BIRTH['cross'][1]
    return [(0, BIRTH['first']), BIRTH['cross']] + [(a, a + 2) for a in range(k, nz, 2)]


def birth_masks():
    """the active mask after each birth (`full` is all ones)"""
    shape = BOXES[BIRTH['box']][0]
    out, m = [], np.zeros(shape, dtype=bool)
    for k0, k1 in birth_layers():
        m = m.copy()
        m[:, :, k0:k1] = True
        out.append(m)
    return out


def birth_dt():
    return BIRTH['cfl'] * DX * DX / KAPPA


# the head of the second half of part 5: waam.run_layer_birth with a recorder on three bricks along axis 2
HEAD = dict(shape=(20, 18, 40), planes_per_layer=2, bead_width=4e-3, scan_speed=0.08, tail=3.0, theta=0.5, cfl=2.0, Ts=1500.0,
            h=300.0, levels=(1450.0, 1395.0, 1440.0))


def head_plan(waam):
    c = HEAD
    full = waam.synthetic_head_mask(*c['shape'])
    layers = waam.plan_layers(full, c['planes_per_layer'])
    tb = waam.birth_times(full, layers, DX, bead_width=c['bead_width'], scan_speed=c['scan_speed'])
    t_out = [tb[-1] + c['tail'] * (tb[-1] - tb[-2])]
    dt_cap = c['cfl'] * DX * DX / KAPPA
    sched = list(waam.layer_birth_schedule(tb, t_out))
    nsubs = [max(1, int(math.ceil(a / dt_cap))) for w, a in sched if w == 'advance']
    return full, layers, tb, t_out, sched, dt_cap, nsubs


def layer_birth_by_single_steps(mod, waam, full, dx, mat_args, h, Tinf, Ts, theta, dt_cap, layers, sched, levels, uint8=None,
                                summary=None):
    """the event loop of waam.run_layer_birth with a recorder, written with the module's own device calls for births and packs
    (mod.birth_planes, grid.set_mask_device on the range, BirthPacks.update), single steps without a recorder, and the
    definition -> (T as NumPy, steps, state, pools, times, mask).  uint8: the dtype of a device mask (torch.uint8; this module
    does not import torch).  summary: optional callable(grid, mask) run after every birth"""
    TH = mod.ThermalHistory
    shape = full.shape
    mask = np.zeros(shape, dtype=bool)
    grid, mat = mod.Grid3D(*shape, dx, mask), mod.Material(*mat_args)
    T = mod.to_device(np.full(shape, Tinf))
    d_full = grid.layout.to_layout(full, uint8)
    d_act = grid.layout.empty(uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    bpacks = mod.BirthPacks(grid, mat, robin_h={f: h for f in FACES})
    packs = bpacks.packs
    state = TH.seed_reference(hc.empty_state(shape), np.asarray(T), mask)
    pools, times, t, steps = [], [], 0.0, 0
    for what, arg in sched:
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = mod.Params(max(arg / nsub, 1e-15), theta)
            run = nsub >= waam.GRAPH_MIN_NSUB
            t0 = t
            for i in range(nsub):
                Tn = mod.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
                t_n = t0 + i * prm.dt if run else t                 # the graph path counts from the run's start
                state, pool = TH.record_reference(state, np.asarray(T), np.asarray(Tn), mask, t_n, prm.dt, levels)
                t = t0 + (i + 1) * prm.dt if run else t_n + prm.dt
                pools.append(pool)
                times.append(t)
                T = Tn
            steps += nsub
        elif what == 'advance':
            t = t + arg                                              # nothing active yet: the global time moves on all the same
        elif what == 'birth':
            ks, ke = layers[arg]
            mod.birth_planes(T, d_act, d_full, grid, ks, ke + 1, Ts)
            grid.set_mask_device(d_act, ks - 1 if ks > 0 else 0, min(shape[2], ke + 2), all_solid=False)
            packs = bpacks.update(ks - 1, ke + 2)
            old = mask.copy()
            mask[:, :, ks:ke + 1] |= full[:, :, ks:ke + 1]
            state = TH.seed_reference(state, np.asarray(T), mask, mask & ~old)
            if summary is not None:
                summary(grid, mask)
    return np.asarray(T), steps, state, pools, times, mask


# ---- 6. a long run through the graph ----------------------------------------------------------------------------------------------
LONG_RUN = dict(shape=(16, 16, 32), steps=401, t0=1.5, h=3000.0, theta=0.5, late=300)
LONG_RUN_DT = 0.12 * DX * DX / KAPPA


def long_run_inputs():
    """(mask, T0, dt): a hot body with a hotter blob across the seam at plane 16, Robin on every face, cooling slowly enough
    that cells are still crossing T_hi and T_lo after step 300"""
    shape = LONG_RUN['shape']
    mask = np.ones(shape, dtype=bool)
    T0 = np.full(shape, 900.0)
    T0[3:13, 3:13, 8:24] = 1900.0
    return mask, T0, LONG_RUN_DT


def late_crossings(states, late):
    """cells whose t_hi / t_lo changed after step `late`"""
    a, b = states[late], states[-1]
    diff = lambda x, y: ~((x == y) | (np.isnan(x) & np.isnan(y)))
    return int(diff(a[1], b[1]).sum()), int(diff(a[2], b[2]).sum())
