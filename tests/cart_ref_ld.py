"""tests/cart_ref_ld.py -- TEST INFRASTRUCTURE.  Extended-precision (np.longdouble) restatement of the Cartesian masked-voxel
theta-step, written from the equations (adi3d_numba_coeff.py:57-118 for the coefficients, :240-302 for
the step).  It shares no code with oracle/adi_oracle.c or oracle/adi_oracle.py: it is the reference the float64 oracle is
itself measured against (tests/test_cart_ref_cpu.py) and the reference of the increment tests over the range of time steps
(tests/cart_dt_cases.py, tests/test_cart_increment_gpu.py).

One step, gamma = k dt / (rho cp dx^2):
    R0 = T + (1 - theta) gamma sum_axes sum_{in-mask neighbours n along the axis} (T_n - T)        on in-mask cells,
then one sweep along axis 0, 1, 2 in turn.  A sweep row of an in-mask cell that is not a Dirichlet cell is
    (e + p + q) x_i - p x_{i-1} - q x_{i+1} = d,    e = 1 + dt coeff,   d = in + dt qflux + dt coeff Tinf,
    p = theta gamma if the lower neighbour is in the mask else 0,  q likewise for the upper neighbour;
a Dirichlet cell is the row x = dir_value (its neighbours still couple to it); an off-mask cell is the row x = in with no
coupling from either side.  So whole grid lines are solved without compaction and the gaps decouple by themselves.  coeff
and qflux of an axis are  h dx^2 / (rho cp dx^3)  and  q dx^2 / (rho cp dx^3)  summed over the exposed faces of that axis; a
face is exposed where the neighbour across it is off the mask or outside the box.

The rows are of the form cyl_ref_ld.thomas_excess solves without a subtraction (e >= 1, p, q >= 0), so the result keeps the
relative precision of np.longdouble at any gamma.

The module has the operator surface helpers.run_cart_case drives (Grid3D, Material, Params,
precompute_coeff_packs_unified, adi_step_numba_coeff); fields come back as np.longdouble arrays."""
import types

import numpy as np

from cyl_ref_ld import thomas_excess

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "cart_ref_ld needs an extended-precision np.longdouble (x87: 64-bit significand)"
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')


def _ld(x):
    return np.asarray(x, dtype=LD)


def _sl(axis, s):
    out = [slice(None)] * 3
    out[axis] = s
    return tuple(out)


def neighbour_in_mask(mask, axis, plus):
    """True where the cell is in the mask and so is its neighbour at +1 (plus) or -1 along `axis`"""
    mask = np.asarray(mask, dtype=bool)
    nb = np.zeros_like(mask)
    if plus:
        nb[_sl(axis, slice(None, -1))] = mask[_sl(axis, slice(1, None))]
    else:
        nb[_sl(axis, slice(1, None))] = mask[_sl(axis, slice(None, -1))]
    return mask & nb


def exposed(mask, face):
    if face not in FACES:
        raise ValueError("bad face")
    axis, plus = divmod(FACES.index(face), 2)
    return np.asarray(mask, dtype=bool) & ~neighbour_in_mask(mask, axis, bool(plus))


# ---- the operator surface ------------------------------------------------------------------------------------------------
def Grid3D(nx, ny, nz, dx, mask):
    mask = np.array(mask, dtype=bool)
    assert mask.shape == (nx, ny, nz)
    return types.SimpleNamespace(nx=nx, ny=ny, nz=nz, dx=dx, mask=mask)


def Material(rho, cp, k):
    return types.SimpleNamespace(rho=rho, cp=cp, k=k)


def Params(dt, theta=0.5):
    return types.SimpleNamespace(dt=dt, theta=theta)


def _face_value(spec, face, shape):
    """a scalar, a per-voxel array, or a dict of either per face -> longdouble array or scalar, None where the face has none"""
    if isinstance(spec, dict):
        spec = spec.get(face)
    if spec is None:
        return None
    v = _ld(spec)
    assert v.ndim == 0 or v.shape == shape
    return v


def precompute_coeff_packs_unified(grid, mat, dir_mask=None, dir_value=None, neumann=None, robin_h=None, robin_Tinf=None):
    """three packs (coeff, qflux, dir_mask, dir_val); robin_Tinf is accepted and ignored, as in the reference"""
    shape = (grid.nx, grid.ny, grid.nz)
    for spec in (neumann, robin_h):
        if isinstance(spec, dict) and any(f not in FACES for f in spec):
            raise ValueError("bad face")
    dx = LD(grid.dx)
    per_area = (dx * dx) / (LD(mat.rho) * LD(mat.cp) * (dx * dx * dx))
    dm = np.zeros(shape, bool) if dir_mask is None else np.array(dir_mask, dtype=bool)
    dv = np.zeros(shape, LD) if dir_value is None else np.array(np.broadcast_to(_ld(dir_value), shape))
    packs = []
    for axis in range(3):
        coeff = np.zeros(shape, LD); qflux = np.zeros(shape, LD)
        for face in FACES[2 * axis: 2 * axis + 2]:
            exp = exposed(grid.mask, face)
            for spec, into in ((robin_h, coeff), (neumann, qflux)):
                v = _face_value(spec, face, shape)
                if v is not None:
                    into += np.where(exp, v * per_area, LD(0))
        packs.append(types.SimpleNamespace(coeff=coeff, qflux=qflux, dir_mask=dm, dir_val=dv))
    return tuple(packs)


def explicit_rhs(T, mask, g_expl):
    """T + g_expl * (sum over the in-mask neighbours of an in-mask cell of T_n - T)"""
    T = _ld(T)
    L = np.zeros(T.shape, LD)
    for axis in range(3):
        lo, hi = _sl(axis, slice(None, -1)), _sl(axis, slice(1, None))
        both = mask[lo] & mask[hi]                           # the pair (i, i + 1) along the axis, both in the mask
        diff = np.where(both, T[hi] - T[lo], LD(0))
        L[lo] += diff
        L[hi] -= diff
    return T + g_expl * L


def sweep(axis, stage_in, mask, tg, dt, pack, Tinf):
    dirc = mask & pack.dir_mask
    free = mask & ~dirc
    dtc = LD(dt) * pack.coeff
    e = np.where(free, 1 + dtc, LD(1))
    d = np.where(free, stage_in + LD(dt) * pack.qflux + dtc * LD(Tinf), np.where(dirc, pack.dir_val, stage_in))
    p = np.where(free & neighbour_in_mask(mask, axis, False), tg, LD(0))
    q = np.where(free & neighbour_in_mask(mask, axis, True), tg, LD(0))
    mv = lambda a: np.moveaxis(a, axis, -1)
    return np.moveaxis(thomas_excess(mv(p), mv(q), mv(e), mv(d)), -1, axis)


def adi_step_numba_coeff(Tn, grid, mat, params, packs, Tinf=0.0, return_stages=False):
    mask = np.asarray(grid.mask, dtype=bool)
    dx = LD(grid.dx)
    gamma = LD(mat.k) / (LD(mat.rho) * LD(mat.cp)) * LD(params.dt) / (dx * dx)
    theta = LD(params.theta)
    R0 = explicit_rhs(Tn, mask, (1 - theta) * gamma)
    U = sweep(0, R0, mask, theta * gamma, params.dt, packs[0], Tinf)
    V = sweep(1, U, mask, theta * gamma, params.dt, packs[1], Tinf)
    W = sweep(2, V, mask, theta * gamma, params.dt, packs[2], Tinf)
    if return_stages:
        return W, dict(R0=R0, U=U, V=V, W=W)
    return W
