"""Shared by tests/test_matlaw_cpu.py and tests/test_matlaw_gpu.py: the steel-like tables, the masks, the loop
    theta = Theta(T) -> theta* = adi_step_numba_coeff(theta, ...) -> T = law.recover(T, theta*, mask, dir_mask)
over any module with the reference's operator surface (the pinned C oracle in the tests), with Robin by h_of * robin_ratio fields,
and the bar problem with its fine explicit reference.  Nothing here needs a GPU."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')

STEEL_T = [20.0, 400.0, 800.0, 1200.0, 1450.0, 1500.0, 2500.0]
STEEL_K = [52.0, 44.0, 30.0, 28.0, 32.0, 60.0, 60.0]
STEEL_CP = [450.0, 560.0, 800.0, 650.0, 700.0, 800.0, 800.0]
STEEL_L, STEEL_TS, STEEL_TL = 2.7e5, 1450.0, 1500.0
RHO = 7800.0


def steel(cls, **kw):
    return cls(STEEL_T, STEEL_K, STEEL_CP, latent_heat=STEEL_L, T_solidus=STEEL_TS, T_liquidus=STEEL_TL, **kw)


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def holes_mask():
    """the 9 x 7 x 11 mask of tests/golden/phase_holes.npz: partial bricks, odd rows"""
    with np.load(os.path.join(HERE, 'golden', 'phase_holes.npz')) as z:
        return np.array(z['mask'])


def seam_mask():
    """20 x 18 x 33: more than one brick along every axis, voids across the brick seams, an off-mask slab"""
    s = (20, 18, 33)
    rng = np.random.default_rng(41)
    mask = rng.random(s) > 0.12
    mask[14:18, 13:17, 14:19] = False                    # a void across the seams at 16
    mask[:, :, 30:] &= rng.random((20, 18, 3)) > 0.5     # a ragged top
    mask[0:3, 0:2, :] = True                             # whole rows
    return mask


def dir_cells(mask, seed=5):
    """about 5 % of the in-mask cells, and a value for each spread over the whole table"""
    rng = np.random.default_rng(seed)
    dm = (rng.random(mask.shape) > 0.95) & mask
    dv = rng.uniform(-50.0, 2800.0, mask.shape)
    return dm, dv


def field_over_the_law(law, mask, seed=3):
    """T with cells in every interval of the law, at its knots, on both linear ends; off the mask planted markers"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(-100.0, 3000.0, mask.shape)
    flat = T.reshape(-1)
    idx = np.flatnonzero(mask.reshape(-1))
    pts = np.concatenate([law.x, 0.5 * (law.x[1:] + law.x[:-1]), [law.x[0] - 70.0, law.x[-1] + 400.0],
                          np.nextafter(law.x, -np.inf), np.nextafter(law.x, np.inf)])
    assert idx.size >= pts.size
    flat[idx[:: idx.size // pts.size][:pts.size]] = pts
    T[~mask] = -12345.5
    return T


def robin_fields(law, loss, T, Tinf):
    """the reference's robin_h for a step from T under `loss` (None: none): h_of * robin_ratio per face"""
    if loss is None:
        return None
    r = law.robin_ratio(T, Tinf)
    return {f: loss.h_of(T, f, Tinf) * r for f in FACES}


def loop_step(orc, law, grid, prm, T, Tinf, rho=RHO, robin=None, dm=None, dv=None, neumann=None, S=None):
    """one step of THE loop over `orc`.  robin: dict face -> h field already times robin_ratio, or None;  dv: Dirichlet values as
    temperatures;  S: a source field [W/m^3] (it enters through the flux of sweep 0, as energy: over rho cp_ref)"""
    mask = np.asarray(grid.mask, dtype=bool)
    mat = orc.Material(rho, law.cp_ref, law.k_ref)
    packs = orc.precompute_coeff_packs_unified(grid, mat, dir_mask=dm, dir_value=None if dv is None else law.theta(dv),
                                               neumann=neumann, robin_h=robin)
    if S is not None:
        packs[0].qflux = packs[0].qflux + np.where(mask, S, 0.0) / (rho * law.cp_ref)
    th = np.where(mask, law.theta(T), T)
    ths = orc.adi_step_numba_coeff(th, grid, mat, prm, packs, Tinf=float(law.theta(float(Tinf))))
    return law.recover(T, ths, mask, dm), ths, packs


# ---- the bar: 200 cells of 0.2 mm, the wall cell held at 2000, the bulk at 20, the far end adiabatic, 0.5 s ------------------
BAR = dict(n=200, dx=2e-4, T_wall=2000.0, T_init=20.0, t_end=0.5)
# "monotone, within [20, 2000]" up to rounding: a cell at rest gets theta* = Theta(20) to a few units in the last place of the
# sweeps' arithmetic and is put back a few 1e-14 off 20.  1e-12 T_wall is 4000 units in the last place of 2000 and nine orders
# below the kelvins by which an unstable or overshooting step breaks either property
BAR_SLACK = 1e-12 * 2000.0


def bar_setup(ny=1):
    """(shape, mask, T0, dir_mask, dir_value): ny x ny lines of n cells along axis 2, the wall cell k = 0 Dirichlet"""
    b = BAR
    shape = (ny, ny, b['n'])
    T0 = np.full(shape, b['T_init'])
    T0[:, :, 0] = b['T_wall']
    dm = np.zeros(shape, dtype=bool)
    dm[:, :, 0] = True
    return shape, np.ones(shape, dtype=bool), T0, dm, np.full(shape, b['T_wall'])


def bar_run(orc, law, nsteps, theta, ny=1):
    shape, mask, T, dm, dv = bar_setup(ny)
    grid = orc.Grid3D(*shape, BAR['dx'], mask)
    prm = orc.Params(BAR['t_end'] / nsteps, theta)
    for _ in range(nsteps):
        T, _, _ = loop_step(orc, law, grid, prm, T, 0.0, dm=dm, dv=dv)
    return T


_bar_ref = {}


def bar_reference(law):
    """the same spatial scheme integrated explicitly in the enthalpy at cfl 0.2 of its stability limit
    dt <= dx^2 rho min(c_eff) / (2 k_ref): H += dt k_ref lap(Theta) / (rho dx^2), T = H^-1(H); computed once"""
    key = law.key()
    if key not in _bar_ref:
        b = BAR
        dt_max = 0.5 * b['dx'] ** 2 * RHO * law.c_eff_min / law.k_ref
        nsteps = int(np.ceil(b['t_end'] / (0.2 * dt_max)))
        dt = b['t_end'] / nsteps
        T = np.full(b['n'], b['T_init'])
        T[0] = b['T_wall']
        H = law.enthalpy(T)
        g = dt * law.k_ref / (RHO * b['dx'] ** 2)
        for _ in range(nsteps):
            th = law.theta(T)
            lap = np.empty_like(th)
            lap[1:-1] = th[2:] - 2.0 * th[1:-1] + th[:-2]
            lap[-1] = th[-2] - th[-1]                      # adiabatic end
            lap[0] = 0.0                                   # the wall is held
            H = H + g * lap
            T = law.enthalpy_inv(H)
        T.setflags(write=False)
        _bar_ref[key] = T
    return _bar_ref[key]
