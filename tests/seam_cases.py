"""Shared by tests/test_loss_phase_seams_cpu.py and tests/test_loss_phase_seams_gpu.py: the boxes, masks, fields, laws and
directed inputs that take k_surface_loss and k_phase_apply / k_phase_seed across the borders of their 16 x 16 x 16 bricks, through
plane ranges that cut bricks, and onto the branch points of the two laws.  Nothing here is stored: every expected value comes
from the pinned C oracle (oracle.adi_oracle) and the NumPy definitions SurfaceLoss.h_of and PhaseChange.correct / f_eq.

The law classes are passed in (`hip.SurfaceLoss`, `hip.PhaseChange`, ...), so this module imports neither the device module
nor torch."""
import math

import numpy as np

import surface_loss_cases as slc
from helpers import rel_linf  # noqa: F401  (re-exported: the project's metric)
from phase_cases import CP, K, KAPPA, RHO  # noqa: F401
from surface_loss_cases import FACES  # noqa: F401

BRICK = 16
DX, TINF = 1e-3, 25.0
MARKER = 7.0

# name -> (logical shape, forced physical box or None: the box the library picks)
BOXES = {
    'S1': ((20, 18, 40), None),            # partial bricks on all axes, three bricks along axis 2 (the last: 8 planes)
    'S1p': ((20, 18, 40), (32, 32, 48)),   # the same inside a box of whole 16-byte rows
    'S2': ((33, 33, 64), None),            # inner bricks (1, 1, 1) and (1, 1, 2)
    'S3': ((17, 17, 19), None),            # odd nz, one-cell-wide last bricks
}
# what the tests rely on, asserted from grid.layout by every test that builds the box
LAYOUT = {
    'S1': dict(padded=False, pz16=8, sx16=0, pz2=0),
    'S1p': dict(padded=True, pz16=0, sx16=0, pz2=0),
    'S2': dict(padded=False, pz16=0, sx16=0, pz2=0),
    'S3': dict(padded=False, pz16=3, sx16=3, pz2=1),
}


def assert_layout(name, layout):
    want = LAYOUT[name]
    px, py, pz, sx = layout.pd
    got = dict(padded=layout.padded, pz16=pz % 16, sx16=sx % 16, pz2=pz % 2)
    assert got == want, (name, layout.pd, got, want)
    if BOXES[name][1] is not None:
        assert (px, py, pz) == BOXES[name][1], (name, layout.pd)


# ---- masks ------------------------------------------------------------------------------------------------------------------
# cavities of the S1 block: (i0, i1, j0, j1, k0, k1), half-open.  Single cells on planes 15, 16, 31, 32, 0 and 39, two of them
# with one cell between them on plane 31; 2 x 2 x 3
# cavities across planes 14-16 and 30-32, one through the brick corner at i = j = 16, one open to the top of the box
S1_CAVITIES = [(5, 6, 5, 6, 15, 16), (10, 11, 9, 10, 16, 17), (3, 4, 12, 13, 31, 32), (14, 15, 4, 5, 32, 33),
               (7, 8, 7, 8, 0, 1), (18, 19, 16, 17, 39, 40), (16, 17, 10, 11, 17, 18), (6, 7, 12, 13, 30, 31), (6, 7, 12, 13, 32, 33),
               (8, 10, 3, 5, 14, 17), (12, 14, 12, 14, 30, 33), (15, 17, 15, 17, 20, 23), (1, 3, 8, 10, 37, 40)]
S2_CAVITY = (22, 25, 22, 25, 22, 25)       # 3 x 3 x 3, wholly inside brick (1, 1, 1)


def _carve(mask, cavities):
    for i0, i1, j0, j1, k0, k1 in cavities:
        mask[i0:i1, j0:j1, k0:k1] = False
    return mask


def mask_of(name, cavity=True):
    shape = BOXES[name][0]
    if name in ('S1', 'S1p'):
        return _carve(np.ones(shape, dtype=bool), S1_CAVITIES)
    if name == 'S2':
        return _carve(np.ones(shape, dtype=bool), [S2_CAVITY] if cavity else [])
    return np.random.default_rng(1703).random(shape) >= 0.25


def exposed_along(mask, axis):
    """in the mask and a neighbour along `axis` missing (the edge of the box counts as missing)"""
    m = np.pad(mask, 1)
    sl = lambda d: tuple(slice(1 + (d if i == axis else 0), 1 + (d if i == axis else 0) + mask.shape[i]) for i in range(3))
    return mask & ~(m[sl(-1)] & m[sl(+1)])


def plane_ranges(name):
    """the [k0, k1) of part 1: whole box, first plane, across / inside / between the brick borders, the last partial brick,
    the last plane, an empty range"""
    nz = BOXES[name][0][2]
    if nz == 40:
        return [(0, nz), (0, 1), (15, 17), (16, 32), (17, 18), (31, 33), (30, nz), (nz - 1, nz), (5, 5)]
    assert nz == 19
    return [(0, nz), (0, 1), (15, 17), (16, nz), (17, 18), (14, 16), (nz - 1, nz), (5, 5)]


# ---- the surface-loss side --------------------------------------------------------------------------------------------------
TABLE5 = ([25.0, 300.0, 700.0, 1100.0, 1500.0], [0.0, 4.0, 9.0, 7.5, 12.0])


def loss5(SurfaceLoss):
    """h, emissivity and a 5-knot table on all faces"""
    return SurfaceLoss(h={f: 8.0 + 1.5 * n for n, f in enumerate(FACES)}, emissivity={f: 0.9 - 0.1 * n for n, f in enumerate(FACES)},
                       table=TABLE5)


def field_of(shape, seed=7):
    """a smooth field plus noise that spans the table (and leaves it at both ends)"""
    x, y, z = [(np.arange(n) + 0.5) / n for n in shape]
    X, Y, Z = np.meshgrid(x, y, z, indexing='ij')
    T = 780.0 + 760.0 * np.sin(5.0 * X + 0.4) * np.cos(4.0 * Y - 0.3) * np.cos(7.0 * Z + 0.2)
    return T + np.random.default_rng(seed).uniform(-40.0, 40.0, shape)


def expected_packs(orc, shape, mask, loss, T, Tinf=TINF, neumann=None):
    """the oracle's packs for per-voxel robin_h = h_of(T): what the header promises the device arrays to equal bit for bit"""
    grid, mat = orc.Grid3D(*shape, DX, mask), orc.Material(RHO, CP, K)
    return orc.precompute_coeff_packs_unified(grid, mat, neumann=neumann, robin_h=slc.h_fields(loss, T, Tinf))


def neumann_of(shape):
    """a scalar on 'z+' and a per-cell array on 'x-'"""
    return {'z+': 2e5, 'x-': 1e5 * (1.0 + 0.25 * np.random.default_rng(29).random(shape))}


BIRTH_PLANES = (14, 18)                    # part 1, Neumann through births: these planes start empty and are born at once
T_BIRTH = 1500.0


# knot tables at the ends of what the law takes.  Both are chosen so that at the LAST knot the interior formula
# fp[n-2] + slope[n-2] * (xp[n-1] - xp[n-2]) and the clamp fp[n-1] are different doubles (asserted on the CPU): only then does
# the `>=` of the clamp show in the result.
TABLE2 = ([700.1, 700.1000311], [0.7, 31.79])                       # 2 knots, a slope of 1e6 (999678.46)
TABLE16 = ([30.3 + 97.7 * m for m in range(16)],                    # MAX_KNOTS, rising and falling segments
           [2.1, 3.7, 3.2, 6.9, 6.3, 8.8, 5.1, 9.7, 11.3, 10.9, 14.2, 13.1, 17.7, 15.3, 0.7, 25.2])
KNOT_CASES = [('knots2_celsius', TABLE2, 273.15), ('knots2_kelvin', TABLE2, 0.0),
              ('knots16_celsius', TABLE16, 273.15), ('knots16_kelvin', TABLE16, 0.0)]


def knot_loss(SurfaceLoss, table, T_offset):
    """'x-' carries nothing (so the table is off on that face), 'y-' radiates as a black body without convection, 'y+' has a
    convection coefficient too small to round the table's value away, the others have everything on"""
    h = {'x-': 0.0, 'x+': 11.0, 'y-': 0.0, 'y+': 1e-3, 'z-': 6.0, 'z+': 14.0}
    e = {'x-': 0.0, 'x+': 0.6, 'y-': 1.0, 'y+': 0.0, 'z-': 0.35, 'z+': 0.8}
    return SurfaceLoss(h=h, emissivity=e, table=table, T_offset=T_offset)


def knot_temperatures(table):
    """every knot, one ulp either side, and values below the first and above the last knot"""
    xp = np.asarray(table[0], dtype=np.float64)
    vals = [xp[0] - 3.0, xp[-1] + 3.0, 0.5 * (xp[0] + xp[1])]
    for x in xp:
        vals += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    return np.array(vals, dtype=np.float64)


def tile(values, shape, shift=0):
    """values[(n + shift) % len] at the n-th cell of a C-ordered array of `shape`"""
    n = int(np.prod(shape))
    return np.asarray(values)[(np.arange(n) + shift) % len(values)].reshape(shape)


def last_knot_doubles(loss, face, Tinf, interior):
    """h_of at the last knot for `face`, with the clamp (interior = False: the definition) or with the last segment's
    interior formula in its place -- the lines of SurfaceLoss.h_of"""
    hs, es, xp, fp, off = loss.validate(Tinf)
    i = FACES.index(face)
    T = xp[-1]
    Tk, Ta = T + off, float(Tinf) + off
    rad = ((es[i] * loss.SIGMA) * (Tk * Tk + Ta * Ta)) * (Tk + Ta)
    slope = (fp[-1] - fp[-2]) / (xp[-1] - xp[-2])
    tab = fp[-2] + slope * (T - xp[-2]) if interior else fp[-1]
    if hs[i] == 0.0 and es[i] == 0.0:
        tab = 0.0
    return (hs[i] + tab) + rad


# ---- the latent-heat side ---------------------------------------------------------------------------------------------------
# the heat capacity of part 4 and the solidus of the two laws whose solidus is free: fl(cp * Ts) / cp != Ts (asserted on the CPU),
# so a cell with H == Hs exactly gets another T from the solid branch (H / cp) than from the mushy one (Ts + 0 / cm).  With the
# usual law's Ts = 1400 the two agree for any cp near 490, so there the `<=` is not observable.
CP_BRANCH, TS_BRANCH = 490.3, 1400.1
F_VALUES = [0.0, -0.0, 1.0, 5e-324, 1.0 - 2.0 ** -53, 0.5, 1.0000000000000002, -1e-3]


def branch_laws(PhaseChange):
    ts = TS_BRANCH
    return [('usual', PhaseChange(2.7e5, 1400.0, 1450.0)),
            ('narrow', PhaseChange(2.7e5, ts, float(np.nextafter(np.nextafter(ts, np.inf), np.inf)))),
            ('ratio', PhaseChange(1e9, ts, ts + 1e-3))]


def _exact_T(cp, L, f, H):
    """a double T with cp*T + L*f == H exactly (the kernel's two products and one sum), or None"""
    t = (H - L * f) / cp
    lo = t
    for _ in range(8):
        lo = np.nextafter(lo, -np.inf)
    for _ in range(17):
        if cp * lo + L * f == H:
            return float(lo)
        lo = np.nextafter(lo, np.inf)
    return None


def branch_table(law, cp=CP_BRANCH):
    """(T*, f) pairs on and around every comparison of the correction: T* in {Ts, Tl, the solutions of cp*T* + L*f == Hs and
    == Hl for every f of F_VALUES} and each of these +-1 and +-2 ulp, crossed with F_VALUES"""
    L, Ts, Tl = law.validate()
    dT, Hs, Hl, cm = law.constants(cp)
    base = {Ts, Tl}
    for f in F_VALUES:
        for H in (Hs, Hl):
            t = _exact_T(cp, L, f, H)
            if t is not None:
                base.add(t)
    temps = set()
    for t in base:
        lo = hi = t
        temps.add(t)
        for _ in range(2):
            lo, hi = float(np.nextafter(lo, -np.inf)), float(np.nextafter(hi, np.inf))
            temps.update((lo, hi))
    temps = sorted(temps)
    Tt = np.repeat(np.array(temps, dtype=np.float64), len(F_VALUES))
    ft = np.tile(np.array(F_VALUES, dtype=np.float64), len(temps))
    return Tt, ft


PHASE_BOXES = {'S3': (17, 17, 19), 'solid': (16, 16, 32)}     # scalar loads / 16-byte loads with all-solid bricks


def branch_inputs(law, box, cp=CP_BRANCH):
    """(mask, dir_mask, T*, f as loaded: 0 off the mask) -- the branch table tiled over the box, the Dirichlet cells and (on S3)
    the holes falling on table entries at other offsets in every repetition"""
    shape = PHASE_BOXES[box]
    Tt, ft = branch_table(law, cp)
    mask = mask_of('S3') if box == 'S3' else np.ones(shape, dtype=bool)
    dm = np.random.default_rng(47).random(shape) < 0.12
    T = tile(Tt, shape)
    f = np.where(mask, tile(ft, shape), 0.0)
    return mask, dm, T, f


def branch_census(law, mask, dm, T, f, cp=CP_BRANCH):
    """how many active cells take each path of the correction, and how many sit exactly on a comparison"""
    L, Ts, Tl = law.validate()
    dT, Hs, Hl, cm = law.constants(cp)
    act = mask & ~dm
    rest_s, rest_l = act & (f == 0.0) & (T <= Ts), act & (f == 1.0) & (T >= Tl)
    go = act & ~rest_s & ~rest_l
    H = cp * T + L * f
    return dict(rest_solid=int(rest_s.sum()), rest_liquid=int(rest_l.sum()), solid=int((go & (H <= Hs)).sum()),
                liquid=int((go & (H >= Hl)).sum()), mushy=int((go & (H > Hs) & (H < Hl)).sum()),
                on_Hs=int((go & (H == Hs)).sum()), on_Hl=int((go & (H == Hl)).sum()),
                rest_on_Ts=int((rest_s & (T == Ts)).sum()), rest_on_Tl=int((rest_l & (T == Tl)).sum()),
                neg_zero=int((act & (f == 0.0) & np.signbit(f)).sum()), outside=int((act & ((f < 0.0) | (f > 1.0))).sum()),
                dirichlet=int((mask & dm).sum()), off_mask=int((~mask).sum()))


# ---- part 3: deposition on a multi-brick head with everything on ------------------------------------------------------------
HEAD = dict(shape=(20, 18, 40), planes_per_layer=3, bead_width=4e-3, scan_speed=0.016, tail=6.0, theta=0.5, cfl=2.0, Ts=1500.0,
            h=15.0, emissivity=0.8, law=(2.7e5, 1400.0, 1450.0))


def head_plan(waam):
    """(full mask, layers, birth times, output times, sub-steps of every segment the run steps through)"""
    c = HEAD
    full = waam.synthetic_head_mask(*c['shape'])
    layers = waam.plan_layers(full, c['planes_per_layer'])
    tb = waam.birth_times(full, layers, DX, bead_width=c['bead_width'], scan_speed=c['scan_speed'])
    t_out = [tb[-1] + c['tail'] * (tb[-1] - tb[-2])]
    dt_cap = c['cfl'] * DX * DX / KAPPA
    sched = list(waam.layer_birth_schedule(tb, t_out))
    first = [w for w, _ in sched].index('birth')                       # (nothing is stepped while nothing is active)
    nsubs = [max(1, int(math.ceil(a / dt_cap))) for w, a in sched[first:] if w == 'advance']
    return full, layers, tb, t_out, nsubs


_head = {}


def head_oracle(orc, waam, SurfaceLoss, PhaseChange):
    """the event loop of waam.run_layer_birth written over the oracle: h_fields lagged, law.correct after every step.  Computed
    once.  -> dict(T, f, steps, melted, mushy, refroze, birth_starts)"""
    if _head:
        return _head
    c = HEAD
    shape = c['shape']
    full, layers, tb, t_out, _ = head_plan(waam)
    loss, law = SurfaceLoss(h=c['h'], emissivity=c['emissivity']), PhaseChange(*c['law'])
    dt_cap = c['cfl'] * DX * DX / KAPPA
    mask = np.zeros(shape, dtype=bool)
    grid, mat = orc.Grid3D(*shape, DX, mask), orc.Material(RHO, CP, K)
    T, f = np.full(shape, TINF), np.zeros(shape)
    steps, was_liquid, refroze, mushy, f_max = 0, np.zeros(shape, dtype=bool), 0, 0, 0.0
    for what, arg in waam.layer_birth_schedule(tb, t_out):
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = orc.Params(max(arg / nsub, 1e-15), c['theta'])
            for _ in range(nsub):
                packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=slc.h_fields(loss, T, TINF))
                T, f = law.correct(orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=TINF), f, mask, None, CP)
                was_liquid |= f == 1.0
                mushy = max(mushy, int(((f > 0.0) & (f < 1.0)).sum()))
                f_max = max(f_max, float(f.max()))
            steps += nsub
        elif what == 'birth':
            ks, ke = layers[arg]
            born = np.zeros(shape, dtype=bool)
            born[:, :, ks:ke + 1] = full[:, :, ks:ke + 1]
            T[born & ~mask] = c['Ts']
            f[born & ~mask] = law.f_eq(np.float64(c['Ts']))
            was_liquid |= born & (f == 1.0)
            mask |= born
            grid.mask = mask.copy()
    refroze = int((was_liquid & mask & (f == 0.0)).sum())
    T.setflags(write=False)
    f.setflags(write=False)
    _head.update(T=T, f=f, steps=steps, f_max=f_max, mushy=mushy, refroze=refroze, birth_starts=[ks for ks, _ in layers],
                 layers=layers)
    return _head


# the 8-step segment of part 3 on S1p: a Goldak source travelling up axis 2 through plane 32, on the face x = nx
SEGMENT = dict(nsteps=8, cfl=2.0, theta=0.5, T0=900.0)


def segment_source(GoldakSource):
    dt = SEGMENT['cfl'] * DX * DX / KAPPA
    v = 3.0 * DX / (SEGMENT['nsteps'] * dt)                          # 3 cells over the run: from plane 30 to plane 33
    return GoldakSource(power=900.0, eta=0.8, a=3e-3, b=3e-3, c_f=3e-3, c_r=6e-3, f_f=0.6,
                        origin=(20 * DX, 9 * DX, 30.5 * DX), velocity=v, travel_axis=2, travel_sign=1, depth_axis=0)


_segment = {}


def segment_oracle(orc, SurfaceLoss, PhaseChange, GoldakSource):
    """the lagged, corrected loop with the moving source over the oracle on the S1 block; computed once -> dict(T0, T, f)"""
    if _segment:
        return _segment
    c = SEGMENT
    shape = BOXES['S1p'][0]
    mask = mask_of('S1p')
    dt = c['cfl'] * DX * DX / KAPPA
    loss, law = SurfaceLoss(h=HEAD['h'], emissivity=HEAD['emissivity']), PhaseChange(*HEAD['law'])
    src = segment_source(GoldakSource)
    go, mato, prmo = orc.Grid3D(*shape, DX, mask), orc.Material(RHO, CP, K), orc.Params(dt, c['theta'])
    T0 = np.where(mask, c['T0'], TINF)
    T, f = T0, law.f_eq(T0) * mask
    centres = []
    for i in range(c['nsteps']):
        po = orc.precompute_coeff_packs_unified(go, mato, robin_h=slc.h_fields(loss, T, TINF))
        po[0].qflux = po[0].qflux + src.sample(go, i * dt + 0.5 * dt) / (RHO * CP)
        centres.append(float(src.center(i * dt + 0.5 * dt)[2]) / DX)
        T, f = law.correct(orc.adi_step_numba_coeff(T, go, mato, prmo, po, Tinf=TINF), f, mask, None, CP)
    for a in (T0, T, f):
        a.setflags(write=False)
    _segment.update(T0=T0, T=T, f=f, centres=centres, mask=mask, dt=dt)
    return _segment
