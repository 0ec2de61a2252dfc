#!/usr/bin/env python3
"""Generate tests/golden/surface_loss_*.npz by IMPORTING THE REFERENCE (build machine only; the reference never travels).

    python tests/golden/make_golden_surface_loss.py --ref <directory of the reference> [--only CASE]

The reference freezes robin_h when the packs are built, but it accepts per-voxel robin_h per face
(adi3d_numba_coeff.py:80-99).  A lagged temperature-dependent coefficient is therefore a loop the reference itself runs:

    for every step:  h_f = law(T)  for the six faces
                     packs = precompute_coeff_packs_unified(grid, mat, dir_mask, dir_value, neumann, robin_h={f: h_f})
                     T = adi_step_numba_coeff(T, grid, mat, params, packs, Tinf)

`law` below restates the five lines of SurfaceLoss.h_of on its own (this file imports nothing of the package):
    Tk = T + T_offset;  Ta = Tinf + T_offset
    rad = ((eps*SIGMA) * (Tk*Tk + Ta*Ta)) * (Tk + Ta)
    tab = fp[j] + ((fp[j+1]-fp[j])/(xp[j+1]-xp[j])) * (T - xp[j])   for xp[j] <= T < xp[j+1], end values outside;
          only on faces whose h or emissivity is non-zero
    h = (h_face + tab) + rad

Every case is a list of segments; a segment starts with an optional birth (planes [k0, k1) of axis 2 of `full_mask` join the
mask at temperature Ts), has its own dt and takes `nsteps` steps.  Stored per case: the inputs; seg<s>_coeff_<axis> -- the
reference's coefficient arrays for the field at the START of the segment (after the birth), at every cell; seg<s>_T<n> --
the field after step n of the segment; h_first_<face> / h_last_<face> and coeff_last_<axis> -- the six h fields of the very
first and the very last step and the last step's coefficient arrays.  A case whose file would pass 900 KB keeps its h fields
in surface_loss_<case>_h_first.npz / _h_last.npz.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
SIGMA = 5.670374419e-8
RHO, CP, K = 7800.0, 490.0, 54.0
KAPPA = K / (RHO * CP)


def law(T, h_face, eps, table, T_offset, Tinf):
    Tk = T + T_offset
    Ta = Tinf + T_offset
    rad = ((eps * SIGMA) * (Tk * Tk + Ta * Ta)) * (Tk + Ta)
    tab = np.zeros_like(T)
    if table is not None and (h_face != 0.0 or eps != 0.0):
        xp, fp = table
        for j in range(len(xp) - 1):
            sel = (xp[j] <= T) & (T < xp[j + 1])
            tab[sel] = fp[j] + ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])) * (T[sel] - xp[j])
        tab[T < xp[0]] = fp[0]
        tab[T >= xp[-1]] = fp[-1]
    return (h_face + tab) + rad


def per_face(spec):
    return np.array([float(spec.get(f, 0.0)) if isinstance(spec, dict) else float(spec) for f in FACES])


def case_holes():
    rng = np.random.default_rng(20261)
    shape = (9, 7, 11)
    mask = rng.random(shape) > 0.30
    mask[:, :, 0] = True                                   # the Dirichlet plane is solid
    dx = 1e-3
    dir_mask = np.zeros(shape, dtype=bool)
    dir_mask[:, :, 0] = True
    return dict(mask=mask, T0=20.0 + 1480.0 * rng.random(shape), dx=dx, theta=0.5, Tinf=25.0,
                h={'x-': 12.0, 'x+': 30.0, 'y-': 0.0, 'y+': 8.5, 'z-': 20.0, 'z+': 15.0},
                emissivity={'x-': 0.8, 'x+': 0.35, 'y-': 0.6, 'y+': 0.9, 'z+': 1.0},          # ('z-' missing: 0)
                table=None, T_offset=273.15, dir_mask=dir_mask, dir_value=150.0 + 10.0 * rng.random(shape),
                neumann={'x+': 4.0e4}, segments=[dict(dt=0.7 * dx * dx / KAPPA, nsteps=4)])


def case_long():
    rng = np.random.default_rng(20262)
    shape = (37, 6, 70)
    mask = np.ones(shape, dtype=bool)
    mask[10:29, 2:4, 20:52] = False                        # one internal void
    dx = 5e-4
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    T0 = 760.0 + 700.0 * np.sin(0.31 * i + 0.2) * np.cos(0.17 * k) * np.cos(0.9 * j) + 30.0 * rng.random(shape)
    return dict(mask=mask, T0=np.clip(T0, 20.0, 1500.0), dx=dx, theta=1.0, Tinf=20.0, h=10.0, emissivity=0.7, table=None,
                T_offset=273.15, dir_mask=None, dir_value=None, neumann=None,
                segments=[dict(dt=200.0 * dx * dx / KAPPA, nsteps=6)])


def case_birth():
    rng = np.random.default_rng(20263)
    shape = (8, 8, 12)
    full = np.ones(shape, dtype=bool)
    full[0, :, 6:] = False                                 # the upper part is narrower than the base ...
    full[:, 7, 8:] = False
    full[3:5, 3:5, 7:11] = False                           # ... and holds a cavity that a later birth closes
    full[6, 1:3, 9] = False
    mask = full.copy()
    mask[:, :, 6:] = False
    dx = 1e-3
    T0 = np.where(mask, 200.0 + 900.0 * rng.random(shape), 25.0)
    dts = [0.6, 0.9, 0.45, 1.3]
    segs = [dict(dt=dts[0] * dx * dx / KAPPA, nsteps=3)]
    for s, (k0, k1) in enumerate([(6, 8), (8, 10), (10, 12)]):
        segs.append(dict(dt=dts[s + 1] * dx * dx / KAPPA, nsteps=3, birth=(k0, k1)))
    return dict(mask=mask, full_mask=full, Ts=1450.0, T0=T0, dx=dx, theta=0.5, Tinf=25.0, h=18.0, emissivity=0.85, table=None,
                T_offset=273.15, dir_mask=None, dir_value=None, neumann=None, segments=segs)


def case_table():
    rng = np.random.default_rng(20264)
    shape = (6, 5, 9)
    mask = rng.random(shape) > 0.15
    xp = np.array([100.0, 400.0, 900.0, 1300.0])
    fp = np.array([6.0, 14.5, 41.0, 38.0])
    T0 = 20.0 + 1480.0 * rng.random(shape)
    T0[0, :, 0] = 100.0                                    # exactly on the knots
    T0[1, :, 1] = 400.0
    T0[2, :, 2] = 900.0
    T0[3, :, 3] = 1300.0
    T0[4, :, 4] = 99.999                                   # below the first knot
    T0[5, :, 5] = 1300.0000001                             # above the last
    dx = 1e-3
    return dict(mask=mask, T0=T0, dx=dx, theta=0.5, Tinf=30.0, h={'x-': 5.0, 'x+': 5.0, 'y-': 2.5, 'z-': 7.0, 'z+': 11.0},
                emissivity=0.0, table=(xp, fp), T_offset=273.15, dir_mask=None, dir_value=None, neumann=None,
                segments=[dict(dt=0.8 * dx * dx / KAPPA, nsteps=2)])      # ('y+' has no h: no table there either)


def case_plain():
    rng = np.random.default_rng(20265)
    shape = (6, 5, 9)
    mask = rng.random(shape) > 0.2
    dx = 1e-3
    return dict(mask=mask, T0=20.0 + 1480.0 * rng.random(shape), dx=dx, theta=0.5, Tinf=30.0,
                h={'x-': 410.0, 'x+': 37.5, 'y+': 999.0, 'z-': 12.25, 'z+': 500.0}, emissivity=0.0, table=None,
                T_offset=273.15, dir_mask=None, dir_value=None, neumann=None,
                segments=[dict(dt=0.8 * dx * dx / KAPPA, nsteps=2)])


CASES = dict(holes=case_holes, long=case_long, birth=case_birth, table=case_table, plain=case_plain)


def run(ref, c):
    shape = c['mask'].shape
    h6, e6 = per_face(c['h']), per_face(c['emissivity'])
    grid = ref.Grid3D(*shape, c['dx'], c['mask'])
    mat = ref.Material(RHO, CP, K)
    mask = c['mask'].copy()
    T = np.array(c['T0'], dtype=np.float64)
    out = dict(mask=c['mask'], T0=T.copy(), dx=np.float64(c['dx']), theta=np.float64(c['theta']), Tinf=np.float64(c['Tinf']),
               rho=np.float64(RHO), cp=np.float64(CP), k=np.float64(K), h=h6, emissivity=e6,
               T_offset=np.float64(c['T_offset']), nseg=np.int64(len(c['segments'])),
               has_table=np.bool_(c['table'] is not None), has_dir=np.bool_(c['dir_mask'] is not None),
               neumann_on=np.array([c['neumann'] is not None and f in c['neumann'] for f in FACES]),
               neumann_q=np.array([float(c['neumann'][f]) if c['neumann'] is not None and f in c['neumann'] else 0.0
                                   for f in FACES]))
    if c['table'] is not None:
        out['table_T'], out['table_h'] = c['table']
    if c['dir_mask'] is not None:
        out['dir_mask'], out['dir_value'] = c['dir_mask'], c['dir_value']
    if 'full_mask' in c:
        out['full_mask'], out['Ts'] = c['full_mask'], np.float64(c['Ts'])

    def h_fields():
        return {f: law(T, h6[i], e6[i], c['table'], c['T_offset'], c['Tinf']) for i, f in enumerate(FACES)}

    def packs_for(hf):
        return ref.precompute_coeff_packs_unified(grid, mat, dir_mask=c['dir_mask'], dir_value=c['dir_value'],
                                                  neumann=c['neumann'], robin_h=hf)
    first = True
    for s, seg in enumerate(c['segments']):
        k0, k1 = seg.get('birth', (-1, -1))
        if k0 >= 0:                                        # activate_layer, waam_from_stl_v7_mm.py:487-495
            newborn = c['full_mask'].copy()
            newborn[:, :, :k0] = False
            newborn[:, :, k1:] = False
            newborn &= ~mask
            T[newborn] = c['Ts']
            mask |= newborn
            grid.mask = mask.copy()
        prm = ref.Params(seg['dt'], c['theta'])
        out['seg%d_dt' % s], out['seg%d_nsteps' % s] = np.float64(seg['dt']), np.int64(seg['nsteps'])
        out['seg%d_k0' % s], out['seg%d_k1' % s] = np.int64(k0), np.int64(k1)
        for n in range(seg['nsteps']):
            hf = h_fields()
            packs = packs_for(hf)
            if n == 0:
                for ax, p in zip('xyz', packs):
                    out['seg%d_coeff_%s' % (s, ax)] = p.coeff.copy()
                if s == 0:
                    out['qflux_x'], out['qflux_y'], out['qflux_z'] = (p.qflux.copy() for p in packs)
            if first:
                for f in FACES:
                    out['h_first_' + f] = hf[f].copy()
                first = False
            T = ref.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=c['Tinf'])
            out['seg%d_T%d' % (s, n + 1)] = T.copy()
    for f in FACES:
        out['h_last_' + f] = hf[f].copy()
    for ax, p in zip('xyz', packs):
        out['coeff_last_' + ax] = p.coeff.copy()
    return out


def save(name, out):
    path = os.path.join(HERE, 'surface_loss_%s.npz' % name)
    np.savez_compressed(path, **out)
    if os.path.getsize(path) > 900 * 1024:
        for part in ('h_first', 'h_last'):
            keys = [k for k in out if k.startswith(part + '_')]
            np.savez_compressed(os.path.join(HERE, 'surface_loss_%s_%s.npz' % (name, part)), **{k: out.pop(k) for k in keys})
        np.savez_compressed(path, **out)
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith('surface_loss_%s' % name) and fn.endswith('.npz'):
            print('wrote', fn, os.path.getsize(os.path.join(HERE, fn)), 'bytes', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default=os.environ.get('ADI_REFERENCE_DIR'), help='directory of the reference (adi3d_numba_coeff.py)')
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    if not a.ref:
        ap.error('give --ref or set ADI_REFERENCE_DIR')
    sys.path.insert(0, a.ref)
    import adi3d_numba_coeff as ref
    for name, make in CASES.items():
        if a.only and a.only != name:
            continue
        save(name, run(ref, make()))


if __name__ == '__main__':
    main()
