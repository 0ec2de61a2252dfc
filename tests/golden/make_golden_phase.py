#!/usr/bin/env python3
"""Generate tests/golden/phase_*.npz by IMPORTING THE REFERENCE (build machine only; the reference never travels).

    python tests/golden/make_golden_phase.py --ref <directory of the reference> [--only CASE]

The reference's step has constant cp.  Latent heat by temperature recovery is a loop over it:

    for every step:  T* = adi_step_numba_coeff(T, grid, mat, params, packs, Tinf)
                     (T, f) = correct(T*, f)

`correct` below restates the law on its own (this file imports nothing of the package).  With dT = Tl - Ts, Hs = cp*Ts,
Hl = cp*Tl + L, cm = cp + L/dT, for every in-mask cell that is not a Dirichlet cell:
    at rest (f == 0 and T* <= Ts, or f == 1 and T* >= Tl): untouched
    else  H = cp*T* + L*f
          H <= Hs: T = H/cp, f = 0;   H >= Hl: T = (H - L)/cp, f = 1;   else T = Ts + (H - Hs)/cm, f = clamp((T - Ts)/dT)
The liquid fraction starts at f_eq(T0) = clamp((T0 - Ts)/dT) on the mask (Dirichlet cells included), 0 off it.

A case is a list of segments, each with its own dt, step count and optional volumetric source field S [W/m^3]; the reference has
no source argument, so S enters as qflux of the axis-0 pack, S/(rho cp), which its sweep adds as dt*qflux to the right-hand side.
Stored per case: the inputs, f0, and per step n (counted over the whole run) Tstar<n>, T<n>, f<n>; `counts`, the number of
cell-visits per branch over the run: at rest solid, at rest liquid, refrozen to f = 0, fully melted, mushy.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
RHO, CP, K = 7800.0, 490.0, 54.0
KAPPA = K / (RHO * CP)
LATENT, TS, TL = 2.7e5, 1400.0, 1450.0


def clamp01(x):
    return np.minimum(np.maximum(x, 0.0), 1.0)


def correct(Tstar, f, active, counts):
    """active: in the mask and not a Dirichlet cell.  counts (5 integers) is advanced by this step's cell-visits."""
    dT = TL - TS
    Hs = CP * TS
    Hl = CP * TL + LATENT
    cm = CP + LATENT / dT
    T, fn = Tstar.copy(), f.copy()
    rest_s = active & (f == 0.0) & (Tstar <= TS)
    rest_l = active & (f == 1.0) & (Tstar >= TL)
    go = active & ~rest_s & ~rest_l
    H = CP * Tstar + LATENT * f
    solid = go & (H <= Hs)
    liquid = go & ~solid & (H >= Hl)
    mushy = go & ~solid & ~liquid
    T[solid] = H[solid] / CP
    fn[solid] = 0.0
    T[liquid] = (H[liquid] - LATENT) / CP
    fn[liquid] = 1.0
    T[mushy] = TS + (H[mushy] - Hs) / cm
    fn[mushy] = clamp01((T[mushy] - TS) / dT)
    for n, sel in enumerate((rest_s, rest_l, solid, liquid, mushy)):
        counts[n] += int(sel.sum())
    return T, fn


def case_holes():
    rng = np.random.default_rng(20301)
    shape = (9, 7, 11)
    mask = rng.random(shape) > 0.30
    mask[:, :, 0] = True                                   # the Dirichlet plane is solid
    dir_mask = np.zeros(shape, dtype=bool)
    dir_mask[:, :, 0] = True
    T0 = 900.0 + 1100.0 * rng.random(shape)
    dir_value = 1380.0 + 100.0 * rng.random(shape)         # Dirichlet cells inside the freezing range
    dx = 1e-3
    return dict(mask=mask, T0=T0, dx=dx, theta=0.5, Tinf=25.0, h=500.0, dir_mask=dir_mask, dir_value=dir_value,
                segments=[dict(dt=0.7 * dx * dx / KAPPA, nsteps=6)], need_all_branches=True)


def case_two_bricks():
    shape = (20, 18, 35)
    mask = np.ones(shape, dtype=bool)
    mask[3:6, 2:5, 20:24] = False                          # a void in the brick (0, 0, 1): its flags are loaded
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    r2 = (i - 15.5) ** 2 + (j - 15.5) ** 2 + (k - 15.5) ** 2      # a blob over the brick corner (16, 16, 16)
    T0 = np.where(r2 <= 4.5 ** 2, 1900.0 - 12.0 * r2, 300.0)
    dx = 1e-3
    return dict(mask=mask, T0=np.where(mask, T0, 25.0), dx=dx, theta=0.5, Tinf=25.0, h=40.0, dir_mask=None, dir_value=None,
                segments=[dict(dt=1.5 * dx * dx / KAPPA, nsteps=3)], need_all_branches=False)


def case_refreeze():
    shape = (16, 16, 32)
    mask = np.ones(shape, dtype=bool)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    r2 = (i - 7.5) ** 2 + (j - 7.5) ** 2 + (k - 22.5) ** 2        # the source sits in the second brick along axis 2
    dx = 1e-3
    S = np.where(r2 <= 2.0 ** 2, 2.5e10, 0.0)                       # W/m^3
    dt = 1.0 * dx * dx / KAPPA
    return dict(mask=mask, T0=np.full(shape, 1250.0), dx=dx, theta=0.5, Tinf=25.0, h=0.0, dir_mask=None, dir_value=None,
                segments=[dict(dt=dt, nsteps=2, S=S), dict(dt=4.0 * dt, nsteps=4), dict(dt=dt, nsteps=2, S=S)],
                need_all_branches=False, liquid_after_segment=[True, False, True])


CASES = dict(holes=case_holes, two_bricks=case_two_bricks, refreeze=case_refreeze)


def run(ref, c):
    shape = c['mask'].shape
    grid = ref.Grid3D(*shape, c['dx'], c['mask'])
    mat = ref.Material(RHO, CP, K)
    has_dir = c['dir_mask'] is not None
    active = c['mask'] & ~c['dir_mask'] if has_dir else c['mask'].copy()
    T = np.array(c['T0'], dtype=np.float64)
    f = np.where(c['mask'], clamp01((T - TS) / (TL - TS)), 0.0)
    out = dict(mask=c['mask'], T0=T.copy(), f0=f.copy(), dx=np.float64(c['dx']), theta=np.float64(c['theta']),
               Tinf=np.float64(c['Tinf']), h=np.float64(c['h']), rho=np.float64(RHO), cp=np.float64(CP), k=np.float64(K),
               latent_heat=np.float64(LATENT), T_solidus=np.float64(TS), T_liquidus=np.float64(TL), has_dir=np.bool_(has_dir),
               nseg=np.int64(len(c['segments'])))
    if has_dir:
        out['dir_mask'], out['dir_value'] = c['dir_mask'], c['dir_value']
    counts = [0] * 5
    n = 0
    for s, seg in enumerate(c['segments']):
        prm = ref.Params(seg['dt'], c['theta'])
        out['seg%d_dt' % s], out['seg%d_nsteps' % s] = np.float64(seg['dt']), np.int64(seg['nsteps'])
        out['seg%d_has_S' % s] = np.bool_('S' in seg)
        packs = ref.precompute_coeff_packs_unified(grid, mat, dir_mask=c['dir_mask'], dir_value=c['dir_value'], neumann=None,
                                                   robin_h={fc: c['h'] for fc in FACES})
        if 'S' in seg:
            out['seg%d_S' % s] = seg['S']
            packs[0].qflux = packs[0].qflux + np.where(c['mask'], seg['S'], 0.0) / (RHO * CP)
        for _ in range(seg['nsteps']):
            Tstar = ref.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=c['Tinf'])
            T, f = correct(Tstar, f, active, counts)
            n += 1
            out['Tstar%d' % n], out['T%d' % n], out['f%d' % n] = Tstar.copy(), T.copy(), f.copy()
        if 'liquid_after_segment' in c:                    # the pool is there / has frozen completely
            assert bool(f.max() > 0.0) == c['liquid_after_segment'][s], (s, float(f.max()))
    out['nsteps'] = np.int64(n)
    out['counts'] = np.array(counts, dtype=np.int64)
    print('branch counts (rest solid, rest liquid, refrozen, melted, mushy):',
          counts, 'max f', float(f.max()), 'max T', float(T.max()), flush=True)
    if c['need_all_branches']:
        assert all(v > 0 for v in counts), counts
    return out


def save(name, out):
    path = os.path.join(HERE, 'phase_%s.npz' % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000 * 1024, (name, size)
    print('wrote', os.path.basename(path), size, 'bytes', flush=True)


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
