"""Temperature-dependent surface loss: the law `SurfaceLoss` and the packs it rewrites in place, `LossPacks`."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from .fields import _native_f64, _p, _stream
from .packs import precompute_coeff_packs_unified, _face_spec


# ---- temperature-dependent surface loss: radiation, h(T) tables (include/adi_hip.h) ------------
class SurfaceLoss:
    """Surface loss that depends on the cell's own temperature: per face a constant convection coefficient `h`, grey-body
    radiation with `emissivity` linearised about the ambient, and an optional piecewise-linear table h(T).
    h, emissivity: a scalar (every face) or a dict face -> scalar over 'x-', 'x+', 'y-', 'y+', 'z-', 'z+' (a missing face: 0,
    as for the reference's robin_h dict).  table: (T_knots, h_values), 2 to 16 strictly increasing knots in the field's unit,
    clamped to the end values outside; it is added on every face whose h or emissivity entry is non-zero.  T_offset: field
    unit -> kelvin.  The ambient of the radiation term is the step's Tinf, the one the Robin term relaxes to.
    The coefficient of a step is evaluated at the cell's temperature at the START of that step (lagged, first order in dt);
    `h_of` is the definition, adi_surface_loss_update the same operations on the device."""
    SIGMA = _lib.SURFACE_LOSS_SIGMA
    MAX_KNOTS = _lib.SURFACE_LOSS_MAX_KNOTS

    def __init__(self, h=0.0, emissivity=0.0, table=None, T_offset=273.15):
        self.h, self.emissivity, self.table, self.T_offset = h, emissivity, table, T_offset
        self.validate()

    @staticmethod
    def _per_face(spec, name):
        if isinstance(spec, dict):
            for f in spec:
                if f not in FACES:
                    raise ValueError("bad face")
            vals = [spec.get(f, 0.0) for f in FACES]
        else:
            vals = [spec] * 6
        try:
            vals = [float(v) for v in vals]
        except (TypeError, ValueError):
            raise ValueError("SurfaceLoss: %s must be a real number or a dict face -> real number" % name)
        if not all(np.isfinite(v) for v in vals):
            raise ValueError("SurfaceLoss: non-finite %s" % name)
        return vals

    def validate(self, Tinf=None):
        """ValueError for anything adi_surface_loss rejects (include/adi_hip.h); with `Tinf`, also an ambient at or below
        0 K.  -> (h[6], emissivity[6], knots, values, T_offset) as floats / float64 arrays"""
        hs = self._per_face(self.h, 'h')
        es = self._per_face(self.emissivity, 'emissivity')
        if min(hs) < 0.0:
            raise ValueError("SurfaceLoss: h < 0")
        if min(es) < 0.0 or max(es) > 1.0:
            raise ValueError("SurfaceLoss: emissivity outside [0, 1]")
        xp = fp = np.zeros(0, dtype=np.float64)
        if self.table is not None:
            try:
                xp, fp = (np.array(v, dtype=np.float64) for v in self.table)
            except (TypeError, ValueError):
                raise ValueError("SurfaceLoss: table must be (T_knots, h_values)")
            if xp.ndim != 1 or xp.shape != fp.shape or xp.size < 2:
                raise ValueError("SurfaceLoss: a table has at least 2 knots and as many values")
            if xp.size > self.MAX_KNOTS:
                raise ValueError("SurfaceLoss: more than %d knots" % self.MAX_KNOTS)
            if not (np.isfinite(xp).all() and np.isfinite(fp).all()):
                raise ValueError("SurfaceLoss: non-finite table entry")
            if not (np.diff(xp) > 0.0).all():
                raise ValueError("SurfaceLoss: knots do not increase")
        off = float(self.T_offset)
        if not np.isfinite(off):
            raise ValueError("SurfaceLoss: non-finite T_offset")
        if Tinf is not None and not float(Tinf) + off > 0.0:
            raise ValueError("SurfaceLoss: Tinf + T_offset <= 0 (the ambient in kelvin)")
        return hs, es, xp, fp, off

    def h_of(self, T, face, Tinf):
        """h [W/m^2/K] on `face` for cell temperatures T (ndarray) and ambient Tinf: THE DEFINITION of the law -- one fp64
        operation per line, in the order the kernel performs them"""
        if face not in FACES:
            raise ValueError("bad face")
        hs, es, xp, fp, off = self.validate(Tinf)
        i = FACES.index(face)
        h_face, eps = hs[i], es[i]
        T = np.asarray(T, dtype=np.float64)
        Tk = T + off
        Ta = float(Tinf) + off
        r1 = eps * self.SIGMA
        r2 = Tk * Tk
        r3 = Ta * Ta
        r4 = r2 + r3
        r5 = r1 * r4
        r6 = Tk + Ta
        rad = r5 * r6
        tab = 0.0
        if xp.size and (h_face != 0.0 or eps != 0.0):
            j = np.clip(np.searchsorted(xp, T, side='right') - 1, 0, xp.size - 2)      # xp[j] <= T < xp[j+1]
            d1 = fp[1:] - fp[:-1]
            d2 = xp[1:] - xp[:-1]
            slope = d1 / d2
            t1 = T - xp[j]
            t2 = slope[j] * t1
            tab = fp[j] + t2
            tab = np.where(T < xp[0], fp[0], tab)
            tab = np.where(T >= xp[-1], fp[-1], tab)
        h1 = h_face + tab
        return h1 + rad

    def as_c(self, Tinf=None):
        hs, es, xp, fp, off = self.validate(Tinf)
        knots = (ctypes.c_double * 16)(*xp)
        vals = (ctypes.c_double * 16)(*fp)
        return _lib.SurfaceLossLaw((ctypes.c_double * 6)(*hs), (ctypes.c_double * 6)(*es), off, int(xp.size), 0, knots, vals)

    def key(self):
        """every parameter of the law: a launch takes it by value, so a captured graph holds the law of its capture"""
        hs, es, xp, fp, off = self.validate()
        return (tuple(hs), tuple(es), tuple(xp.tolist()), tuple(fp.tolist()), off)


class LossPacks:
    """The coefficient packs of a body that loses heat by a SurfaceLoss: `.packs` are three AxisCoeffPack whose Robin
    coefficient arrays are REWRITTEN IN PLACE on the device from the temperature field (adi_surface_loss_update); the sweeps read
    them per voxel on exposed rows, as for any pack built from robin_h arrays.  Dirichlet cells and Neumann fluxes come from one
    ordinary precompute_coeff_packs_unified call here.  The d_coeff pointers never change, so a StagedStepper's graph and the
    no-fallback promise (which depends on the flags, not on coefficient values) survive every update.
        update(T)                  before a step: the exposed cells only; no allocation, no host synchronisation
        rebuild(T, k_begin, k_end) after `grid.mask` changed on those planes of axis 2 (default: the whole box): every cell,
                                   zeros where a cell is no longer exposed; Neumann fluxes of the planes rebuilt as well
    T (optional, here): the field the arrays are evaluated from at once; without it they hold zeros until the first update /
    rebuild, which the step performs itself when it is given `surface_loss=`."""

    def __init__(self, grid, mat, loss, Tinf, dir_mask=None, dir_value=None, neumann=None, T=None):
        if not isinstance(loss, SurfaceLoss):
            raise TypeError("LossPacks: loss must be a SurfaceLoss")
        loss.validate(Tinf)
        self.grid, self.mat, self.loss, self.Tinf = grid, mat, loss, float(Tinf)
        self.packs = precompute_coeff_packs_unified(grid, mat, dir_mask=dir_mask, dir_value=dir_value, neumann=neumann,
                                                    robin_h=None)
        for p in self.packs:
            p.face_consts = None                     # per-voxel coefficients: read on exposed rows (sparse_ok stays True)
        self._coeff = ptr_array([p.d_coeff.data_ptr() for p in self.packs])
        self._qflux = ptr_array([p.d_qflux.data_ptr() for p in self.packs])
        L = grid.layout
        keep = []
        qs = [_face_spec(neumann.get(f) if neumann is not None else None, L, keep) for f in FACES]
        self._has_q = any(q[0] != _lib.FACE_NONE for q in qs)
        self._q_args = ((ctypes.c_int * 6)(*[q[0] for q in qs]), (ctypes.c_double * 6)(*[q[1] for q in qs]),
                        ptr_array([q[2].data_ptr() if q[2] is not None else None for q in qs]), keep)
        self._h_none = ((ctypes.c_int * 6)(*[_lib.FACE_NONE] * 6), (ctypes.c_double * 6)(), ptr_array([None] * 6))
        if T is not None:
            self.rebuild(T)

    def _launch(self, T, Tinf, k0, k1, full):
        g, m = self.grid, self.mat
        t = _native_f64(g, T)                                 # host arrays / foreign tensors: a copy (not the step's path)
        law = self.loss.as_c(self.Tinf if Tinf is None else Tinf)
        check(lib.adi_surface_loss_update(ctypes.byref(law), float(self.Tinf if Tinf is None else Tinf), _p(t), _p(g.d_flags),
                                          _p(g.d_bricks), *g.layout.pd, g.dx, m.rho, m.cp, self._coeff, int(k0), int(k1),
                                          int(full), _stream()))

    def update(self, T, Tinf=None):
        """the per-step mode over the whole box, from the device field T (DeviceField or tensor in the grid's layout);
        Tinf: the step's ambient (default: the one given at construction)"""
        self._launch(T, Tinf, 0, self.grid.layout.pz, 0)
        return self.packs

    def graph_key(self):
        """what a captured launch holds of the loss: the law, by value"""
        return self.loss.key()

    def rebuild(self, T, k_begin=0, k_end=None, Tinf=None):
        """the full mode on the planes [k_begin, k_end) of axis 2 (clipped to the box), for the grid's CURRENT mask"""
        g, m = self.grid, self.mat
        whole = k_end is None and int(k_begin) <= 0
        k0 = max(0, int(k_begin))
        k1 = g.layout.pz if whole else min(g.nz, g.nz if k_end is None else int(k_end))
        if k1 > k0:
            if self._has_q:
                hm, hs, hf = self._h_none
                qm, qs, qf, _ = self._q_args
                check(lib.adi_build_coeffs_planes(_p(g.d_mask), *g.layout.pd, g.dx, m.rho, m.cp, hm, hs, hf, qm, qs, qf,
                                                  self._coeff, self._qflux, k0, min(k1, g.layout.pz), _stream()))
            self._launch(T, Tinf, k0, k1, 1)
        for a, p in enumerate(self.packs):
            p.mask_version = g.mask_version
            p._fractions = (g, a, g.mask_version)
        return self.packs
