"""Deposition helpers: the surface impulse, the perimeter ratio of a voxelised section, and layer births on the device
(`birth_planes`, `BirthPacks`)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from .fields import DeviceField, Grid3D, _device, _p, _stream
from .packs import AxisCoeffPack, _face_constants


def apply_surface_impulse_Q(T, grid, mat, Q, face='z-'):
    """adi3d_numba_coeff.py:304-320: add dT = Q/(rho cp dx) to the in-mask cells of the domain-boundary plane of
    `face`, IN PLACE (NumPy array or DeviceField).  ValueError("bad face") for an unknown face."""
    if face not in FACES:
        raise ValueError("bad face")
    dT = Q / (mat.rho * mat.cp * grid.dx)
    ax, plus = FACES.index(face) // 2, FACES.index(face) % 2
    sl = [slice(None)] * 3
    sl[ax] = -1 if plus else 0
    sl = tuple(sl)
    if isinstance(T, DeviceField):
        sel = (grid.d_mask[sl] != 0)
        plane = T.t[sl]
        plane[sel] = plane[sel] + dT
    else:
        sel = np.asarray(grid.mask)[sl]
        T[sl][sel] += dT


# ---- per-voxel Robin correction: perimeter ratio --------------------------------------------
_LATERAL = ('x-', 'x+', 'y-', 'y+')


def exposed_faces_per_layer(mask_or_grid, faces=_LATERAL):
    """Number of exposed faces (in-mask cell whose neighbour across the face is outside the mask or the box) per plane
    k of axis 2, counted on the device from the neighbour-flags digest: int64 array of length nz.  With the four
    lateral faces this is the digital perimeter of every layer divided by dx."""
    for f in faces:
        if f not in FACES:
            raise ValueError("bad face")
    if isinstance(mask_or_grid, Grid3D):
        g = mask_or_grid
    else:
        m = np.asarray(mask_or_grid)
        g = Grid3D(m.shape[0], m.shape[1], m.shape[2], 1.0, m)
    bits = sum(1 << FACES.index(f) for f in set(faces))
    counts = torch.empty(g.layout.pz, dtype=torch.int64, device=_device())
    check(lib.adi_count_exposed_faces(_p(g.d_flags), *g.layout.pd, bits, _p(counts), _stream()))
    return counts[:g.nz].cpu().numpy()                # (the planes of the physical box beyond nz hold no in-mask cell)


def count_exposed_faces(mask2d):
    """quick_compare_layer_birth_robin_v3.py:97-108: exposed x-/x+/y-/y+ faces of a 2-D section (an integer)."""
    m = np.asarray(mask2d).astype(bool)
    assert m.ndim == 2
    return int(exposed_faces_per_layer(m[:, :, None])[0])


def perimeter_ratio(mask2d, dx, perim_true):
    """gamma = true perimeter / digital perimeter of the voxelised section (quick_compare_layer_birth_robin_v3.py:109-112);
    the lateral Robin coefficient of a staircase surface is scaled by it: h_side_eff = h_side * gamma (pi/4 for a
    large disk)."""
    faces = count_exposed_faces(mask2d)
    if faces == 0:
        raise ValueError("empty section")
    return float(perim_true) / (faces * float(dx))


# ---- layer birth on the device --------------------------------------------------------------
def birth_planes(T, d_active, d_full, grid, k_begin, k_end, Ts, count=None):
    """activate_layer (waam_from_stl_v7_mm.py:487-495) on the planes [k_begin, k_end) of axis 2, one kernel:
    newborn = full & ~active; T[newborn] = Ts; active |= full.  T: DeviceField; d_active / d_full: uint8 tensors in the
    grid's layout.  `count`: optional int64 device tensor (1 element) that receives the number of newborn cells."""
    L = grid.layout
    assert L.is_native(d_active) and L.is_native(d_full) and L.is_native(T.t)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=T.t.device)
    check(lib.adi_birth_planes(_p(T.t), _p(d_active), _p(d_full), *grid.layout.pd, int(k_begin),
                               int(k_end), float(Ts), _p(count), _stream()))
    return count


class BirthPacks:
    """The coefficient packs of a part that grows by layer births along axis 2 (precompute_coeff_packs_unified with
    scalar / None face specifications, no Dirichlet cells), kept in HBM and UPDATED IN PLACE after a birth: only the
    planes of the new layer and the one below / above it change exposure, so the flags and the six coefficient arrays
    are rebuilt on [k_begin - 1, k_end + 1) instead of the whole box -- the same arrays the reference's full rebuild
    (waam_from_stl_v7_mm.py:534) would give."""

    def __init__(self, grid, mat, robin_h=None, neumann=None):
        self.grid, self.mat = grid, mat
        L = grid.layout

        def spec(v):
            if v is None:
                return (_lib.FACE_NONE, 0.0)
            if not np.isscalar(v):
                raise TypeError("BirthPacks takes scalar face specifications (use precompute_coeff_packs_unified for fields)")
            return (_lib.FACE_SCALAR, float(v))
        hs = [spec(None if robin_h is None else (robin_h.get(f, 0.0) if isinstance(robin_h, dict) else robin_h)) for f in FACES]
        qs = [spec(neumann.get(f) if neumann is not None else None) for f in FACES]
        self._args = ((ctypes.c_int * 6)(*[h[0] for h in hs]), (ctypes.c_double * 6)(*[h[1] for h in hs]), ptr_array([None] * 6),
                      (ctypes.c_int * 6)(*[q[0] for q in qs]), (ctypes.c_double * 6)(*[q[1] for q in qs]), ptr_array([None] * 6))
        self.coeff = [L.empty(zero=True) for _ in range(3)]
        self.qflux = [L.empty(zero=True) for _ in range(3)]
        has_q = any(q[0] != _lib.FACE_NONE for q in qs)
        self.packs = tuple(AxisCoeffPack(self.coeff[a], None, None, self.qflux[a], _has_dir=False, _has_q=has_q, _layout=L)
                           for a in range(3))
        fcs = _face_constants(grid, mat, [h[0] for h in hs], [h[1] for h in hs], [q[0] for q in qs], [q[1] for q in qs])
        for a, p in enumerate(self.packs):
            p.sparse_ok = True
            p.face_consts = fcs[a]
        self.update(0, grid.nz)

    def update(self, k_begin, k_end):
        """rebuild the planes [k_begin, k_end) of axis 2 from the grid's current device mask"""
        g, m = self.grid, self.mat
        k0, k1 = max(0, int(k_begin)), min(g.nz, int(k_end))
        hm, hs, hf, qm, qs, qf = self._args
        check(lib.adi_build_coeffs_planes(_p(g.d_mask), *g.layout.pd, g.dx, m.rho, m.cp, hm, hs, hf, qm, qs, qf,
                                          ptr_array([c.data_ptr() for c in self.coeff]),
                                          ptr_array([q.data_ptr() for q in self.qflux]), k0, k1, _stream()))
        for a, p in enumerate(self.packs):
            p.mask_version = g.mask_version
            p._fractions = (g, a, g.mask_version)
        return self.packs
