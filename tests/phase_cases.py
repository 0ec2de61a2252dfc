"""Shared by tests/test_phase_cpu.py and tests/test_phase_gpu.py: the golden cases of tests/golden/make_golden_phase.py (inputs
and the reference's results, read from the .npz files), the loop
    T* = adi_step_numba_coeff(T, ...) -> (T, f) = law.correct(T*, f, mask, dir_mask, cp)
over any module with the reference's operator surface (the pinned C oracle in the tests), and the one-dimensional Stefan problem
with its closed form."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
CASES = ('holes', 'two_bricks', 'refreeze')
RHO, CP, K = 7800.0, 490.0, 54.0
KAPPA = K / (RHO * CP)


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


_cache = {}


def load(name):
    """every array of phase_<name>.npz, read once, never modified"""
    if name not in _cache:
        c = {}
        with np.load(os.path.join(HERE, 'golden', 'phase_%s.npz' % name)) as z:
            for k in z.files:
                c[k] = z[k]
                c[k].setflags(write=False)
        _cache[name] = c
    return _cache[name]


def law_of(c, cls):
    return cls(float(c['latent_heat']), float(c['T_solidus']), float(c['T_liquidus']))


def f_bar(c):
    """the bar on f: the 1e-10 relative bar on T pushed through f = (T - Ts)/dT"""
    return 1e-10 * float(np.abs(c['T0']).max()) / (float(c['T_liquidus']) - float(c['T_solidus']))


def dir_of(c):
    return (np.array(c['dir_mask']), np.array(c['dir_value'])) if bool(c['has_dir']) else (None, None)


def segments(c):
    """[(dt, nsteps, S or None)]"""
    return [(float(c['seg%d_dt' % s]), int(c['seg%d_nsteps' % s]), np.array(c['seg%d_S' % s]) if bool(c['seg%d_has_S' % s]) else None)
            for s in range(int(c['nseg']))]


def robin_of(c):
    return {f: float(c['h']) for f in FACES}


def run_corrected(orc, c, law, visit):
    """the corrected loop of the case over `orc`; visit(n, Tstar, T, f) after step n (1-based, counted over the whole run)"""
    shape = c['mask'].shape
    mask = np.array(c['mask'])
    grid = orc.Grid3D(*shape, float(c['dx']), mask)
    mat = orc.Material(float(c['rho']), float(c['cp']), float(c['k']))
    dm, dv = dir_of(c)
    T, f = np.array(c['T0']), np.array(c['f0'])
    n = 0
    for dt, nsteps, S in segments(c):
        prm = orc.Params(dt, float(c['theta']))
        packs = orc.precompute_coeff_packs_unified(grid, mat, dir_mask=dm, dir_value=dv, robin_h=robin_of(c))
        if S is not None:
            packs[0].qflux = packs[0].qflux + np.where(mask, S, 0.0) / (float(c['rho']) * float(c['cp']))
        for _ in range(nsteps):
            Tstar = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=float(c['Tinf']))
            T, f = law.correct(Tstar, f, mask, dm, float(c['cp']))
            n += 1
            visit(n, Tstar, T, f)
    return T, f


# ---- the Stefan problem: a half-space at T_i < T_m whose wall is held at T_w > T_m from t = 0 ------------------------------
STEFAN = dict(n=300, dx=1e-4, T_wall=1725.0, T_init=1125.0, T_melt=1425.0, half_range=0.5, latent=2.7e5, cfl=2.0, nsteps=452,
              theta=0.5)


def stefan_lambda():
    """lambda of Neumann's solution for equal properties of the two phases:
    St_l / (exp(l^2) erf l) - St_s / (exp(l^2) erfc l) = l sqrt(pi)"""
    from scipy.optimize import brentq
    from scipy.special import erf, erfc
    s = STEFAN
    st_l = CP * (s['T_wall'] - s['T_melt']) / s['latent']
    st_s = CP * (s['T_melt'] - s['T_init']) / s['latent']
    return brentq(lambda l: st_l / (math.exp(l * l) * erf(l)) - st_s / (math.exp(l * l) * erfc(l)) - l * math.sqrt(math.pi),
                  1e-6, 5.0)


def stefan_setup(ny=1):
    """(shape, mask, T0, dir_mask, dir_value, dt): ny x ny lines of n cells along axis 2, the wall cell k = 0 Dirichlet, every
    other face adiabatic"""
    s = STEFAN
    shape = (ny, ny, s['n'])
    T0 = np.full(shape, s['T_init'])
    T0[:, :, 0] = s['T_wall']
    dm = np.zeros(shape, dtype=bool)
    dm[:, :, 0] = True
    return shape, np.ones(shape, dtype=bool), T0, dm, np.full(shape, s['T_wall']), s['cfl'] * s['dx'] * s['dx'] / KAPPA


def stefan_front_error(f_line, n, dt, lam):
    """|numerical - analytic| front position after n steps, in cells: the front is (sum of f beyond the wall cell + 1/2) dx
    from the wall, which sits at the centre of cell 0"""
    num = float(np.sum(f_line[1:])) + 0.5
    return abs(num - 2.0 * lam * math.sqrt(KAPPA * n * dt) / STEFAN['dx'])
