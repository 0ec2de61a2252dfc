"""The coefficient packs of the Cartesian step: `Material`, `Params`, `AxisCoeffPack`, `exposed_mask` and
`precompute_coeff_packs_unified` (adi3d_numba_coeff.py:21-118), built on the device."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from .fields import Layout, DeviceField, _p, _stream


class Material:  # adi3d_numba_coeff.py:21-23
    def __init__(self, rho, cp, k):
        self.rho = float(rho); self.cp = float(cp); self.k = float(k)


class Params:  # adi3d_numba_coeff.py:25-27
    def __init__(self, dt, theta=0.5):
        self.dt = float(dt); self.theta = float(theta)


class AxisCoeffPack:
    """adi3d_numba_coeff.py:29-36.  Arrays live in HBM (`d_*` tensors, device layout); the reference's
    attribute names `.coeff / .dir_mask / .dir_val / .qflux` return host copies (drivers read
    `packs[2].qflux`, quick_compare_neumann_robin.py:104)."""

    def __init__(self, coeff, dir_mask, dir_val, qflux=None, _has_dir=None, _has_q=None, _layout=None):
        self.layout = _layout or Layout(*tuple(coeff.shape))
        L = self.layout
        self.d_coeff = L.to_layout(coeff, torch.float64)
        self.d_dir_mask = None if dir_mask is None else L.to_layout(dir_mask, torch.uint8)
        self.d_dir_val = None if dir_val is None else L.to_layout(dir_val, torch.float64)
        self.d_qflux = None if qflux is None else L.to_layout(qflux, torch.float64)
        if _has_dir is None:
            _has_dir = self.d_dir_mask is not None and bool(self.d_dir_mask.any().item())
        if _has_q is None:
            _has_q = self.d_qflux is not None and bool((self.d_qflux != 0).any().item())
        self.has_dir, self.has_q = bool(_has_dir), bool(_has_q)
        if self.has_dir and self.d_dir_val is None:
            self.d_dir_val = L.empty(zero=True)
        # Set by precompute_coeff_packs_unified only: coeff/qflux are non-zero just on cells exposed along the
        # pack's axis, so the sweep may skip loading them elsewhere.  Hand-built packs are read densely.
        self.sparse_ok = False
        self.face_consts = None        # (c-, c+, q-, q+) when built from per-face scalars (precompute_coeff_packs_unified)
        self._fractions = None         # (grid, axis, mask version) the byte accounting is evaluated from, on demand
        self._exposed_fraction = 1.0   # fraction of cells exposed along the axis
        self._dir_fraction = 1.0

    def _eval_fractions(self):
        if self._fractions is not None:
            grid, a, ver = self._fractions
            self._fractions = None
            if grid.mask_version != ver:       # the mask moved on before anybody asked: keep the dense figures
                return
            fl = grid.d_flags
            L = self.layout
            ncell = float(L.nx * L.ny * L.nz)
            inmask = (fl & 1) == 1
            self._exposed_fraction = float((inmask & (((fl >> (1 + 2 * a)) & 3) != 3)).sum().item()) / ncell
            self._dir_fraction = float(self.d_dir_mask.sum().item()) / ncell if self.has_dir else 0.0

    @property
    def exposed_fraction(self):
        self._eval_fractions()
        return self._exposed_fraction

    @property
    def dir_fraction(self):
        self._eval_fractions()
        return self._dir_fraction

    @property
    def variant(self):
        if self.has_dir:
            return _lib.SWEEP_GENERAL if self.has_q else _lib.SWEEP_NO_Q
        return _lib.SWEEP_NO_DIR if self.has_q else _lib.SWEEP_LEAN

    def _host(self, t, dtype):
        if t is None:
            return np.zeros(self.layout.shape, dtype=dtype)
        return t.cpu().contiguous().numpy().astype(dtype, copy=False)

    @property
    def bytes_per_cell(self):
        """HBM bytes per cell the sweep of this pack must move (its inputs + the output): the byte count of
        the roofline (SURVEY.md 8(d) variant rule)."""
        fe = self.exposed_fraction if self.sparse_ok else 1.0
        if self.sparse_ok and self.face_consts is not None:
            fe = 0.0                                      # per-face scalars: coeff / qflux are not read at all
        b = 8.0 + 1.0 + 8.0 + 8.0 * fe                    # in, flags, out, coeff
        if self.has_q:
            b += 8.0 * fe
        if self.has_dir:
            b += 1.0 + 8.0 * (self.dir_fraction if self.sparse_ok else 1.0)
        return b

    coeff = property(lambda self: self._host(self.d_coeff, np.float64))
    qflux = property(lambda self: self._host(self.d_qflux, np.float64))
    dir_mask = property(lambda self: self._host(self.d_dir_mask, np.bool_))
    dir_val = property(lambda self: self._host(self.d_dir_val, np.float64))


def exposed_mask(mask, face):
    """adi3d_numba_coeff.py:38-55; ValueError("bad face") for an unknown face."""
    if face not in FACES:
        raise ValueError("bad face")
    host = not isinstance(mask, (torch.Tensor, DeviceField))
    shape = tuple(mask.shape)
    assert len(shape) == 3
    L = Layout(*shape, sx=shape[1] * shape[2])
    d = L.to_layout(mask, torch.uint8)
    out = L.empty(torch.uint8)
    check(lib.adi_exposed_mask(_p(d), shape[0], shape[1], shape[2], 0, FACES.index(face), _p(out), _stream()))
    return out.cpu().numpy().astype(np.bool_) if host else out.to(torch.bool)


def _face_spec(spec, L, keep):
    """scalar / array / None -> (mode, scalar, device tensor or None)"""
    if spec is None:
        return (_lib.FACE_NONE, 0.0, None)
    if np.isscalar(spec):
        return (_lib.FACE_SCALAR, float(spec), None)
    t = L.to_layout(spec, torch.float64)
    keep.append(t)
    return (_lib.FACE_FIELD, 0.0, t)


def _face_constants(grid, mat, h_modes, h_scalars, q_modes, q_scalars):
    """per axis (c-, c+, q-, q+) as a ctypes array of 4 doubles, or None where a face of the axis carries a per-voxel field:
    what the sweeps take as `h_face_consts` instead of loading coeff / qflux at the exposed cells (adi_face_constants)"""
    consts = (ctypes.c_double * 12)()
    valid = (ctypes.c_int * 3)()
    check(lib.adi_face_constants(grid.dx, mat.rho, mat.cp, (ctypes.c_int * 6)(*h_modes), (ctypes.c_double * 6)(*h_scalars),
                                 (ctypes.c_int * 6)(*q_modes), (ctypes.c_double * 6)(*q_scalars), consts, valid))
    return [(ctypes.c_double * 4)(*consts[4 * a:4 * a + 4]) if valid[a] else None for a in range(3)]


def _fc_arg(grid, pack, sp):
    """the h_face_consts argument for a sweep of `pack` under the `sparse` word `sp`: only with sparse reads (fresh packs)"""
    fc = getattr(pack, 'face_consts', None)
    return fc if (fc is not None and (sp & 1)) else None


def precompute_coeff_packs_unified(grid, mat, dir_mask=None, dir_value=None, neumann=None,
                                   robin_h=None, robin_Tinf=None):
    """adi3d_numba_coeff.py:57-118: one HIP pass builds the Robin coefficient and Neumann flux fields
    of the three axes on the device.  `robin_Tinf` is accepted and ignored, as in the reference (the
    ambient enters at step time)."""
    L = grid.layout
    d_mask = grid.sync_mask()
    keep = []
    h_specs, q_specs = [], []
    for f in FACES:
        if robin_h is None:
            h_specs.append((_lib.FACE_NONE, 0.0, None))
        elif isinstance(robin_h, dict):
            h_specs.append(_face_spec(robin_h.get(f, 0.0), L, keep))
        else:
            h_specs.append(_face_spec(robin_h, L, keep))
        q_specs.append(_face_spec(neumann.get(f) if neumann is not None else None, L, keep))
    if neumann is not None:
        for f in neumann:
            if f not in FACES:
                raise ValueError("bad face")   # exposed_mask(grid.mask, f) raises in the reference (:106)

    coeff = [L.empty() for _ in range(3)]
    qflux = [L.empty() for _ in range(3)]
    hm = (ctypes.c_int * 6)(*[s[0] for s in h_specs])
    hs = (ctypes.c_double * 6)(*[s[1] for s in h_specs])
    hf = ptr_array([s[2].data_ptr() if s[2] is not None else None for s in h_specs])
    qm = (ctypes.c_int * 6)(*[s[0] for s in q_specs])
    qs = (ctypes.c_double * 6)(*[s[1] for s in q_specs])
    qf = ptr_array([s[2].data_ptr() if s[2] is not None else None for s in q_specs])
    check(lib.adi_build_coeffs(_p(d_mask), *grid.layout.pd, grid.dx, mat.rho, mat.cp,
                               hm, hs, hf, qm, qs, qf,
                               ptr_array([c.data_ptr() for c in coeff]), ptr_array([q.data_ptr() for q in qflux]),
                               _stream()))
    has_q = any(s[0] != _lib.FACE_NONE for s in q_specs)
    d_dm = d_dv = None
    has_dir = False
    if dir_mask is not None:
        d_dm = L.to_layout(dir_mask, torch.uint8)
        has_dir = bool(d_dm.any().item())
        if dir_value is None:
            d_dv = L.empty(zero=True)                                   # :75-76
        elif np.isscalar(dir_value):
            d_dv = L.empty(zero=L.padded)
            d_dv.fill_(float(dir_value))                                # :77-78
        else:
            d_dv = L.to_layout(dir_value, torch.float64)
    packs = tuple(AxisCoeffPack(coeff[a], d_dm, d_dv, qflux[a], _has_dir=has_dir, _has_q=has_q, _layout=L)
                  for a in range(3))
    fcs = _face_constants(grid, mat, [s[0] for s in h_specs], [s[1] for s in h_specs], [s[0] for s in q_specs],
                          [s[1] for s in q_specs])
    for a, p in enumerate(packs):
        p.mask_version = grid.mask_version
        p.sparse_ok = True
        p.face_consts = fcs[a]                           # per-face scalars: the sweeps need not load coeff / qflux
        p._fractions = (grid, a, grid.mask_version)      # exposed / Dirichlet fractions: evaluated when somebody asks
    return packs
