"""tests/matmap_ref_ld.py -- TEST INFRASTRUCTURE.  Extended-precision (np.longdouble) restatement of the Cartesian theta-step on
a grid of several materials, written from the equations (include/adi_hip.h, "Several materials").  It
shares no code with the package: MaterialMap.step_reference (fp64) and the kernels are both measured against it
(tests/matmap_cases.py).

Materials m = (rho, cp, k) with C_m = rho cp; every in-mask cell has an id.  Pair table
    kf(m, m) = k_m,   kf(m, n) = 2 k_m k_n / (k_m + k_n),   G[m][n] = kf(m, n) dt / (C_m dx^2).
Explicit stage on in-mask cells (off the mask R0 = T):
    R0_i = T_i + (1 - theta) sum over in-mask neighbours n of G[id_i][id_n] (T_n - T_i)   [+ dt S_i / C_{id_i}]
then one sweep along axis 0, 1, 2.  The row of a free cell is (e + p + q) x_i - p x_{i-1} - q x_{i+1} = d with
e = 1 + dt coeff, d = in + dt qflux + dt coeff Tinf, p = theta G[id_i][id_{i-1}] where the lower neighbour is in the mask (else
0), q likewise; a Dirichlet cell is x = dir_value; an off-mask cell x = in.  coeff_i = sum over the exposed faces of the axis of
h dx^2 / (C_{id_i} dx^3), qflux alike.  Solved by cyl_ref_ld.thomas_excess (no subtraction)."""
import types

import numpy as np

from cyl_ref_ld import thomas_excess

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "matmap_ref_ld needs an extended-precision np.longdouble"
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')


def _sl(axis, s):
    out = [slice(None)] * 3
    out[axis] = s
    return tuple(out)


def pair_table(materials, dx, dt):
    n = len(materials)
    G = np.zeros((n, n), LD)
    for m, (rho_m, cp_m, k_m) in enumerate(materials):
        for j, (_, _, k_n) in enumerate(materials):
            kf = LD(k_m) if m == j else 2 * LD(k_m) * LD(k_n) / (LD(k_m) + LD(k_n))
            G[m, j] = kf * LD(dt) / (LD(rho_m) * LD(cp_m) * LD(dx) * LD(dx))
    return G


def heat_capacity(materials, ids, mask):
    C = np.array([LD(rho) * LD(cp) for rho, cp, _ in materials], LD)
    return C[np.where(mask, ids, 0).astype(np.intp)]


def _face_value(spec, face):
    if isinstance(spec, dict):
        spec = spec.get(face)
    return None if spec is None else np.asarray(spec, dtype=LD)


def packs(mask, ids, materials, dx, dir_mask=None, dir_value=None, neumann=None, robin_h=None):
    mask = np.asarray(mask, dtype=bool)
    shape = mask.shape
    dx = LD(dx)
    per_area = (dx * dx) / (heat_capacity(materials, ids, mask) * (dx * dx * dx))
    dm = np.zeros(shape, bool) if dir_mask is None else np.array(dir_mask, dtype=bool)
    dv = np.zeros(shape, LD) if dir_value is None else np.array(np.broadcast_to(np.asarray(dir_value, LD), shape))
    out = []
    for axis in range(3):
        coeff = np.zeros(shape, LD); qflux = np.zeros(shape, LD)
        for plus in (0, 1):
            face = FACES[2 * axis + plus]
            nb = np.zeros_like(mask)                      # the neighbour across the face is in the mask
            if plus:
                nb[_sl(axis, slice(None, -1))] = mask[_sl(axis, slice(1, None))]
            else:
                nb[_sl(axis, slice(1, None))] = mask[_sl(axis, slice(None, -1))]
            exp = mask & ~nb
            for spec, into in ((robin_h, coeff), (neumann, qflux)):
                v = _face_value(spec, face)
                if v is not None:
                    into += np.where(exp, v * per_area, LD(0))
        out.append(types.SimpleNamespace(coeff=coeff, qflux=qflux, dir_mask=dm, dir_val=dv))
    return tuple(out)


def explicit(T, mask, idm, G, om, src=None):
    T = np.asarray(T, dtype=LD)
    acc = np.zeros(T.shape, LD)
    for axis in range(3):
        lo, hi = _sl(axis, slice(None, -1)), _sl(axis, slice(1, None))
        both = mask[lo] & mask[hi]                        # the pair (i, i + 1) along the axis, both in the mask
        diff = np.where(both, T[hi] - T[lo], LD(0))
        acc[lo] += G[idm[lo], idm[hi]] * diff
        acc[hi] -= G[idm[hi], idm[lo]] * diff
    R0 = T + om * acc
    if src is not None:
        R0 = R0 + np.where(mask, src, LD(0))
    return R0


def sweep(axis, X, mask, idm, tG, dt, pack, Tinf):
    dirc = mask & np.asarray(pack.dir_mask, dtype=bool)
    free = mask & ~dirc
    dtc = LD(dt) * np.asarray(pack.coeff, dtype=LD)
    e = np.where(free, 1 + dtc, LD(1))
    d = np.where(free, X + LD(dt) * np.asarray(pack.qflux, dtype=LD) + dtc * LD(Tinf),
                 np.where(dirc, np.asarray(pack.dir_val, dtype=LD), X))
    lo, hi = _sl(axis, slice(None, -1)), _sl(axis, slice(1, None))
    both = mask[lo] & mask[hi]
    p = np.zeros(X.shape, LD); q = np.zeros(X.shape, LD)
    p[hi] = np.where(both & free[hi], tG[idm[hi], idm[lo]], LD(0))
    q[lo] = np.where(both & free[lo], tG[idm[lo], idm[hi]], LD(0))
    mv = lambda a: np.moveaxis(a, axis, -1)
    return np.moveaxis(thomas_excess(mv(p), mv(q), mv(e), mv(d)), -1, axis)


def step(T, mask, ids, materials, dx, dt, theta, pk, Tinf, S=None, return_stages=False):
    mask = np.asarray(mask, dtype=bool)
    idm = np.where(mask, ids, 0).astype(np.intp)
    G = pair_table(materials, dx, dt)
    theta = LD(theta)
    src = None if S is None else LD(dt) * np.asarray(S, dtype=LD) / heat_capacity(materials, ids, mask)
    R0 = explicit(T, mask, idm, G, 1 - theta, src)
    U = sweep(0, R0, mask, idm, theta * G, dt, pk[0], Tinf)
    V = sweep(1, U, mask, idm, theta * G, dt, pk[1], Tinf)
    W = sweep(2, V, mask, idm, theta * G, dt, pk[2], Tinf)
    if return_stages:
        return W, dict(R0=R0, U=U, V=V, W=W)
    return W
