"""Shared by tests/test_surface_loss_cpu.py and tests/test_surface_loss_gpu.py: the golden cases of
tests/golden/make_golden_surface_loss.py (inputs and the reference's results, read from the .npz files) and the lagged loop
    h_f = loss.h_of(T, f, Tinf) -> precompute_coeff_packs_unified(robin_h={f: h_f}) -> adi_step_numba_coeff
over any module with the reference's operator surface (the pinned C oracle in the tests)."""
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
CASES = ('holes', 'long', 'birth', 'table', 'plain')


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


_cache = {}


def load(name):
    """every array of surface_loss_<name>.npz and its companions (_h_first, _h_last), read once, never modified"""
    if name not in _cache:
        files = sorted(glob.glob(os.path.join(HERE, 'golden', 'surface_loss_%s.npz' % name)) +
                       glob.glob(os.path.join(HERE, 'golden', 'surface_loss_%s_h_*.npz' % name)))
        assert files, 'no golden vectors for %s' % name
        c = {}
        for fn in files:
            with np.load(fn) as z:
                for k in z.files:
                    c[k] = z[k]
                    c[k].setflags(write=False)
        _cache[name] = c
    return _cache[name]


def loss_of(c, cls):
    table = (c['table_T'], c['table_h']) if bool(c['has_table']) else None
    return cls(h={f: float(v) for f, v in zip(FACES, c['h'])}, emissivity={f: float(v) for f, v in zip(FACES, c['emissivity'])},
               table=table, T_offset=float(c['T_offset']))


def bc_of(c):
    """dir_mask / dir_value / neumann keyword arguments of the case"""
    neumann = {f: float(q) for f, q, on in zip(FACES, c['neumann_q'], c['neumann_on']) if on} or None
    return dict(dir_mask=np.array(c['dir_mask']) if bool(c['has_dir']) else None,
                dir_value=np.array(c['dir_value']) if bool(c['has_dir']) else None, neumann=neumann)


def segments(c):
    """[(s, dt, nsteps, k0, k1)]; k0 < 0: no birth ahead of the segment"""
    return [(s, float(c['seg%d_dt' % s]), int(c['seg%d_nsteps' % s]), int(c['seg%d_k0' % s]), int(c['seg%d_k1' % s]))
            for s in range(int(c['nseg']))]


def born_mask(c, mask, k0, k1):
    """activate_layer (waam_from_stl_v7_mm.py:487-495): the cells of full_mask on planes [k0, k1) that are not active yet"""
    nb = np.array(c['full_mask'])
    nb[:, :, :k0] = False
    nb[:, :, k1:] = False
    return nb & ~mask


def h_fields(loss, T, Tinf):
    return {f: loss.h_of(T, f, Tinf) for f in FACES}


def run_lagged(orc, c, loss, visit):
    """the lagged loop of the case over `orc`; visit(s, n, T, packs) after step n (1-based) of segment s, and with n = 0 for
    the packs of the field at the start of the segment (after its birth)"""
    shape = c['mask'].shape
    mask = np.array(c['mask'])
    grid = orc.Grid3D(*shape, float(c['dx']), mask)
    mat = orc.Material(float(c['rho']), float(c['cp']), float(c['k']))
    Tinf = float(c['Tinf'])
    T = np.array(c['T0'])
    bc = bc_of(c)
    for s, dt, nsteps, k0, k1 in segments(c):
        if k0 >= 0:
            nb = born_mask(c, mask, k0, k1)
            T[nb] = float(c['Ts'])
            mask |= nb
            grid.mask = mask.copy()
        prm = orc.Params(dt, float(c['theta']))
        for n in range(nsteps):
            packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=h_fields(loss, T, Tinf), **bc)
            if n == 0:
                visit(s, 0, T, packs)
            T = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
            visit(s, n + 1, T, packs)
    return T
