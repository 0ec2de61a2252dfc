"""Latent heat of melting and freezing: the law `PhaseChange` and the liquid fraction of a grid, `PhaseField`."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _SeededForMask, _device, _native_f64, _p, _stream


# ---- latent heat of melting and freezing (include/adi_hip.h) -----------------------------------------
class PhaseChange:
    """Latent heat `latent_heat` [J/kg] released between `T_solidus` and `T_liquidus` (the field's unit), linearly in T: on
    the equilibrium curve the liquid fraction is f_eq(T) = min(max((T - Ts)/(Tl - Ts), 0), 1).  The step runs at constant cp
    from the state (T, f); afterwards the cell's enthalpy cp*T + L*f is put back on the curve (temperature recovery: lagged,
    first order in dt).  `correct` is the definition, adi_phase_apply the same operations on the device."""

    def __init__(self, latent_heat, T_solidus, T_liquidus):
        self.latent_heat, self.T_solidus, self.T_liquidus = latent_heat, T_solidus, T_liquidus
        self.validate()

    def validate(self):
        """ValueError for anything adi_phase_change rejects (include/adi_hip.h).  -> (L, Ts, Tl) as floats"""
        try:
            L, Ts, Tl = float(self.latent_heat), float(self.T_solidus), float(self.T_liquidus)
        except (TypeError, ValueError):
            raise ValueError("PhaseChange: latent_heat, T_solidus and T_liquidus must be real numbers")
        if not (np.isfinite(L) and np.isfinite(Ts) and np.isfinite(Tl)):
            raise ValueError("PhaseChange: non-finite parameter")
        if not L > 0.0:
            raise ValueError("PhaseChange: latent_heat must be > 0")
        if not Tl > Ts:
            raise ValueError("PhaseChange: T_liquidus must be above T_solidus")
        return L, Ts, Tl

    def as_c(self):
        return _lib.PhaseChangeLaw(*self.validate())

    def key(self):
        """every parameter of the law: a launch takes it by value, so a captured graph holds the law of its capture"""
        return self.validate()

    def constants(self, cp):
        """(dT, Hs, Hl, cm) for heat capacity cp, each one fp64 operation, as the library's host code evaluates them"""
        L, Ts, Tl = self.validate()
        cp = float(cp)
        if not (np.isfinite(cp) and cp > 0.0):
            raise ValueError("PhaseChange: cp must be finite and > 0")
        dT = Tl - Ts
        Hs = cp * Ts
        h1 = cp * Tl
        Hl = h1 + L
        r = L / dT
        cm = cp + r
        return dT, Hs, Hl, cm

    def f_eq(self, T):
        """the liquid fraction on the equilibrium curve at temperatures T (ndarray)"""
        _, Ts, Tl = self.validate()
        T = np.asarray(T, dtype=np.float64)
        dT = Tl - Ts
        e = T - Ts
        x = e / dT
        x = np.where(x < 0.0, 0.0, x)
        return np.where(x > 1.0, 1.0, x)

    def correct(self, T_star, f, mask, dir_mask, cp):
        """(T, f) after the correction of the step's result T_star from the liquid fraction f it started with: THE DEFINITION
        of the law -- one fp64 operation per line, in the order the kernel performs them.  mask: the grid's mask; dir_mask: the
        Dirichlet cells (None: none).  Off-mask cells, Dirichlet cells and cells at rest keep T_star and f bit for bit."""
        L, Ts, Tl = self.validate()
        dT, Hs, Hl, cm = self.constants(cp)
        cp = float(cp)
        Tst = np.asarray(T_star, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64)
        act = np.asarray(mask, dtype=bool)
        if dir_mask is not None:
            act = act & ~np.asarray(dir_mask, dtype=bool)
        rest = ((f == 0.0) & (Tst <= Ts)) | ((f == 1.0) & (Tst >= Tl))
        act = act & ~rest
        h1 = cp * Tst
        h2 = L * f
        H = h1 + h2
        # H <= Hs: all solid
        Ta = H / cp
        # H >= Hl: all liquid
        d1 = H - L
        Tb = d1 / cp
        # between: on the mushy branch of the curve
        d2 = H - Hs
        q = d2 / cm
        Tc = Ts + q
        e = Tc - Ts
        x = e / dT
        x = np.where(x < 0.0, 0.0, x)
        fc = np.where(x > 1.0, 1.0, x)
        lo, hi = H <= Hs, H >= Hl
        Tn = np.where(lo, Ta, np.where(hi, Tb, Tc))
        fn = np.where(lo, 0.0, np.where(hi, 1.0, fc))
        return np.where(act, Tn, Tst), np.where(act, fn, f)


class PhaseField(_SeededForMask):
    """The liquid fraction of a grid under a PhaseChange law, on the device: `f` (fp64, the grid's layout, 0 off the mask) and
    the phase summary (one word per 16^3 brick, 0 exactly when every f of the brick is 0: adi_phase_apply far from the melt
    pool reads T once and nothing else).  Both buffers live as long as the object, so a StagedStepper's graph holds their
    pointers.  T (optional): the field f is seeded from, f = f_eq(T) on the mask; without it everything is solid.
    dir_mask (optional): the Dirichlet cells of `apply` calls that are not given any (the step passes its pack's).
        apply(T)              the correction on a device field in the grid's layout, T and f in place: one launch
        seed(T, sel=None)     f = f_eq(T) on the in-mask cells `sel` selects (None: all), 0 off the mask
        sync_mask(T)          after `grid.mask` changed: the cells that joined the mask are seeded from T, those that left it
                              are zeroed, every other cell keeps its f
        snapshot() / restore(s), copy_state_from(other)     f and the summary"""

    def __init__(self, grid, mat, law, T=None, dir_mask=None):
        if not isinstance(law, PhaseChange):
            raise TypeError("PhaseField: law must be a PhaseChange")
        law.constants(mat.cp)
        self.grid, self.mat, self.law = grid, mat, law
        L = grid.layout
        self._flat = torch.zeros(L.numel_padded, dtype=torch.float64, device=_device())
        self.f = self._flat.as_strided(L.shape, L.strides)
        self.summary = torch.zeros(self._words(), dtype=torch.int32, device=_device())
        self.d_dir_mask = None if dir_mask is None else L.to_layout(dir_mask, torch.uint8)
        if T is not None:
            self.seed(T)
        else:
            self._remember_mask()

    def _words(self):
        n = int(lib.adi_phase_summary_words(*self.grid.layout.pd[:3]))
        if n <= 0:
            raise ValueError("PhaseField: bad grid")
        return n

    @property
    def liquid_fraction(self):
        """a copy of f as a DeviceField of the grid's shape"""
        return DeviceField(self.f).copy()

    def apply(self, T, d_dir_mask=None):
        """adi_phase_apply on T (a DeviceField or device tensor in the grid's layout), in place; d_dir_mask: the Dirichlet
        cells as a uint8 device tensor in the grid's layout (default: the ones given at construction)"""
        g = self.grid
        t = _native_f64(g, T, "PhaseField.apply: T must be a fp64 device field in the grid's layout (it is corrected in place)")
        if g.mask_version != self._mask_version:
            raise ValueError("PhaseField: the grid's mask changed since the liquid fraction was seeded; call sync_mask(T)")
        assert self.summary.numel() == self._words()
        dm = self.d_dir_mask if d_dir_mask is None else d_dir_mask
        if dm is not None:
            assert g.layout.is_native(dm) and dm.dtype == torch.uint8
        check(lib.adi_phase_apply(ctypes.byref(self.law.as_c()), float(self.mat.cp), _p(t), _p(self.f), _p(g.d_flags),
                                  _p(g.d_bricks), _p(dm), _p(self.summary), *g.layout.pd, _stream()))
        return T

    def seed(self, T, sel=None):
        """adi_phase_seed: f = f_eq(T) on the in-mask cells `sel` selects (bool / uint8 array or tensor of the grid's shape;
        None: every in-mask cell), 0 off the mask; the summary is rewritten"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        assert self.summary.numel() == self._words()
        check(lib.adi_phase_seed(ctypes.byref(self.law.as_c()), _p(_native_f64(g, T)), _p(self.f), _p(g.d_flags), _p(g.d_bricks),
                                 _p(d_sel), _p(self.summary), *g.layout.pd, _stream()))
        self._remember_mask()

    def set_liquid_fraction(self, f):
        """load f (array / tensor / DeviceField of the grid's shape; taken as 0 off the mask) and rebuild the summary from it
        on the device: a seed that selects no cell keeps every in-mask f, zeroes the rest and rewrites every entry"""
        g = self.grid
        self.f.copy_(g.layout.to_layout(f, torch.float64))
        self.seed(g.layout.empty(zero=True), sel=g.layout.empty(torch.uint8, zero=True))

    def snapshot(self):
        return self._flat.clone(), self.summary.clone()

    def restore(self, s):
        self._flat.copy_(s[0])
        self.summary.copy_(s[1])

    def copy_state_from(self, other):
        if other.grid.layout.pd != self.grid.layout.pd:
            raise ValueError("PhaseField.copy_state_from: the grids differ in layout")
        self._flat.copy_(other._flat)
        self.summary.copy_(other.summary)

    def graph_key(self):
        """what a captured graph holds of the field: the law by value, the buffers by pointer"""
        return (self.law.key(), self.f.data_ptr(), self.summary.data_ptr(),
                None if self.d_dir_mask is None else self.d_dir_mask.data_ptr())
