"""Latent heat of melting and freezing: the law `PhaseChange` and the liquid fraction of a grid, `PhaseField`; temperature-dependent
k(T) and cp(T): the law `MaterialLaw` and what a step under it runs with, `NonlinearPacks`."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _SeededForMask, _device, _native_f64, _p, _stream
from .packs import Material
from .surface_loss import SurfaceLoss, LossPacks


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


# ---- temperature-dependent conductivity and heat capacity (include/adi_hip.h) --------------------------
class MaterialLaw:
    """k(T) and cp(T), piecewise-linear in the knots `T` (>= 2, strictly increasing; values finite and > 0) and held at their end
    values outside, with an optional latent heat released linearly between `T_solidus` < `T_liquidus`: the two points are merged
    into the knots (k and cp interpolated there) and latent_heat/(Tl - Ts) is added to cp on the intervals between them, so cp
    may jump at a knot and every interval keeps its own left value and slope.  At most MAX_KNOTS knots after merging.
    Two exact changes of variable carry the law around the linear step:
        Kirchhoff temperature  Theta(T) = x0 + (1/k_ref) int_{x0}^{T} k dT      div(k grad T) = k_ref lap(Theta)
        enthalpy               H(T) = int cp dT + L f_eq(T)                      (per unit mass, H = cp(x0) T below the first knot)
    so the step solves rho dH/dt = k_ref lap(Theta) + q: the linear ADI step on Theta with Material(rho, cp_ref, k_ref), then
    H(T_new) = H(T_old) + cp_ref (Theta* - Theta_old) cell by cell (`recover`: temperature recovery, lagged, first order in
    dt, stateless -- the liquid fraction is f_eq(T)).  Stable exactly when cp_ref <= 2 theta min c_eff, c_eff = dH/dTheta
    = cp(T) k_ref / k(T); the defaults k_ref = k[0], cp_ref = min c_eff keep theta = 0.5 stable and the profile monotone.
    Piece p of the tables is anchored at knot x[p] (left value y, slope s, integral V there); the last piece and the one below
    the first knot have slope 0.  Every method is the definition of a device operation: one fp64 operation per line, in the
    order the kernels of csrc/adi_matlaw_dev.hpp perform them."""
    MAX_KNOTS = _lib.MATLAW_MAX_KNOTS

    def __init__(self, T, k, cp, latent_heat=None, T_solidus=None, T_liquidus=None, k_ref=None, cp_ref=None):
        try:
            x, kv, cv = (np.array(v, dtype=np.float64) for v in (T, k, cp))
        except (TypeError, ValueError):
            raise ValueError("MaterialLaw: T, k and cp must be sequences of real numbers")
        if x.ndim != 1 or x.size < 2 or kv.shape != x.shape or cv.shape != x.shape:
            raise ValueError("MaterialLaw: at least 2 knots, and as many k and cp values")
        if not (np.isfinite(x).all() and np.isfinite(kv).all() and np.isfinite(cv).all()):
            raise ValueError("MaterialLaw: non-finite table entry")
        if not (np.diff(x) > 0.0).all():
            raise ValueError("MaterialLaw: knots do not increase")
        if not ((kv > 0.0).all() and (cv > 0.0).all()):
            raise ValueError("MaterialLaw: k and cp must be > 0")
        latent = (latent_heat, T_solidus, T_liquidus)
        if any(v is not None for v in latent):
            if any(v is None for v in latent):
                raise ValueError("MaterialLaw: latent_heat, T_solidus and T_liquidus come together")
            self.L, self.Ts, self.Tl = PhaseChange(*latent).validate()
            xm = np.union1d(x, np.array([self.Ts, self.Tl]))
            kv, cv, x = np.interp(xm, x, kv), np.interp(xm, x, cv), xm
        else:
            self.L, self.Ts, self.Tl = 0.0, None, None
        n = x.size
        if n > self.MAX_KNOTS:
            raise ValueError("MaterialLaw: more than %d knots%s" % (self.MAX_KNOTS, " after merging" if self.L else ""))
        self.k_ref = float(kv[0] if k_ref is None else k_ref)
        if not (np.isfinite(self.k_ref) and self.k_ref > 0.0):
            raise ValueError("MaterialLaw: k_ref must be finite and > 0")
        self.c_eff_min = float(np.min(cv * self.k_ref / kv))           # (before the latent boost: cp only grows by it)
        self.cp_ref = self.c_eff_min if cp_ref is None else float(cp_ref)
        if not (np.isfinite(self.cp_ref) and self.cp_ref > 0.0):
            raise ValueError("MaterialLaw: cp_ref must be finite and > 0")
        # the per-interval tables, each entry one fp64 operation
        boost = np.zeros(n - 1)
        if self.L:
            r = self.L / (self.Tl - self.Ts)
            boost = np.where((x[:-1] >= self.Ts) & (x[1:] <= self.Tl), r, 0.0)
        d = x[1:] - x[:-1]
        kq = kv / self.k_ref
        ks = np.append((kq[1:] - kq[:-1]) / d, 0.0)
        c = np.append(cv[:-1] + boost, cv[-1])                         # left values; the last piece holds the end value
        cr = cv[1:] + boost                                            # right values of the intervals
        cs = np.append((cr - c[:-1]) / d, 0.0)
        self.n, self.x, self.kq, self.ks, self.c, self.cs, self.c_lo = n, x, kq, ks, c, cs, float(cv[0])
        self.hks, self.hcs = 0.5 * ks, 0.5 * cs                        # (exact)
        self.ks2, self.cs2 = 2.0 * ks, 2.0 * cs                        # (exact)
        th, H = np.empty(n), np.empty(n)
        th[0] = x[0]
        H[0] = self.c_lo * x[0]
        for j in range(n - 1):
            th[j + 1] = self._fwd(x[j + 1], x[j], kq[j], self.hks[j], th[j])
            H[j + 1] = self._fwd(x[j + 1], x[j], c[j], self.hcs[j], H[j])
        self.th, self.H = th, H
        if not (np.isfinite(th).all() and np.isfinite(H).all() and (np.diff(th) > 0.0).all() and (np.diff(H) > 0.0).all()):
            raise ValueError("MaterialLaw: the tables overflow fp64 or do not increase")
        # piece p of a lookup: 0 below the first knot, j + 1 from knot j on
        lo = lambda first, a: np.concatenate(([first], a))             # noqa: E731
        self._xa = lo(x[0], x)
        self._k = (lo(kq[0], kq), lo(0.0, self.hks), lo(0.0, self.ks2), lo(th[0], th), lo(0.0, ks))
        self._c = (lo(self.c_lo, c), lo(0.0, self.hcs), lo(0.0, self.cs2), lo(H[0], H), lo(0.0, cs))

    @staticmethod
    def _fwd(t, xa, y, hs, Va):
        """V(t) on the piece anchored at xa: Va + (y + hs*e)*e with e = t - xa, hs half the slope"""
        e = t - xa
        a1 = hs * e
        a2 = y + a1
        a3 = a2 * e
        return Va + a3

    @staticmethod
    def _inv(V, xa, y, s2, Va):
        """t with V(t) = V on the piece anchored at xa: e = 2 dV / (y + sqrt(y*y + s2*dV)), s2 twice the slope -- no
        cancellation, and e = dV / y where the slope is 0"""
        dV = V - Va
        b1 = y * y
        b2 = s2 * dV
        b3 = b1 + b2
        r = np.sqrt(b3)
        den = y + r
        num = dV + dV
        e = num / den
        return xa + e

    def _piece(self, T):
        T = np.asarray(T, dtype=np.float64)
        return T, np.searchsorted(self.x, T, side='right')

    def _kq_of(self, T):
        T, p = self._piece(T)
        e = T - self._xa[p]
        a1 = self._k[4][p] * e
        return self._k[0][p] + a1

    def k_of(self, T):
        """k(T) [W/m/K]"""
        return self.k_ref * self._kq_of(T)

    def cp_of(self, T):
        """cp(T) [J/kg/K] with the latent boost between T_solidus and T_liquidus; at a knot, the value to its right"""
        T, p = self._piece(T)
        e = T - self._xa[p]
        a1 = self._c[4][p] * e
        return self._c[0][p] + a1

    def f_eq(self, T):
        """the liquid fraction at temperatures T: min(max((T - Ts)/(Tl - Ts), 0), 1); 0 without latent heat"""
        T = np.asarray(T, dtype=np.float64)
        if not self.L:
            return np.zeros_like(T)
        dT = self.Tl - self.Ts
        e = T - self.Ts
        x = e / dT
        x = np.where(x < 0.0, 0.0, x)
        return np.where(x > 1.0, 1.0, x)

    def theta(self, T):
        """the Kirchhoff temperature Theta(T)"""
        T, p = self._piece(T)
        return self._fwd(T, self._xa[p], self._k[0][p], self._k[1][p], self._k[3][p])

    def enthalpy(self, T):
        """H(T) [J/kg]"""
        T, p = self._piece(T)
        return self._fwd(T, self._xa[p], self._c[0][p], self._c[1][p], self._c[3][p])

    def theta_inv(self, V):
        V = np.asarray(V, dtype=np.float64)
        p = np.searchsorted(self.th, V, side='right')
        return self._inv(V, self._xa[p], self._k[0][p], self._k[2][p], self._k[3][p])

    def enthalpy_inv(self, V):
        V = np.asarray(V, dtype=np.float64)
        p = np.searchsorted(self.H, V, side='right')
        return self._inv(V, self._xa[p], self._c[0][p], self._c[2][p], self._c[3][p])

    def min_theta(self):
        """the smallest Params.theta the step is stable with: cp_ref / (2 min c_eff)"""
        return self.cp_ref / (2.0 * self.c_eff_min)

    def material(self, rho):
        """the constant material the linear step on Theta runs with"""
        return Material(rho, self.cp_ref, self.k_ref)

    def robin_ratio(self, T, Tinf):
        """(T - Tinf) / (Theta(T) - Theta(Tinf)), and 1/kq(Tinf) where the denominator is 0: a Robin coefficient times this
        makes the sweeps' sink c (Theta - Theta_inf) the loss h (T - Tinf)"""
        T = np.asarray(T, dtype=np.float64)
        num = T - float(Tinf)
        den = self.theta(T) - float(self.theta(float(Tinf)))
        rinf = 1.0 / float(self._kq_of(float(Tinf)))
        with np.errstate(divide='ignore', invalid='ignore'):
            q = num / den
        return np.where(den == 0.0, rinf, q)

    def recover(self, T_n, theta_star, mask, dir_mask):
        """T at the end of a step from its start T_n and the linear step's result theta_star: THE DEFINITION of the recovery.
        Off-mask cells keep theta_star (there the sweeps passed T_n through); Dirichlet cells (dir_mask, None: none) get
        theta_inv(theta_star); every other in-mask cell puts H(T_n) + cp_ref (theta_star - Theta(T_n)) back on the curve, and
        keeps T_n bit for bit where that difference is 0."""
        T_n = np.asarray(T_n, dtype=np.float64)
        ths = np.asarray(theta_star, dtype=np.float64)
        act = np.asarray(mask, dtype=bool)
        dirc = np.zeros_like(act) if dir_mask is None else (np.asarray(dir_mask, dtype=bool) & act)
        d = ths - self.theta(T_n)
        g = self.cp_ref * d
        Hn = self.enthalpy(T_n) + g
        Tn = np.where(d == 0.0, T_n, self.enthalpy_inv(Hn))
        return np.where(dirc, self.theta_inv(ths), np.where(act, Tn, ths))

    def as_c(self):
        a = lambda v: (ctypes.c_double * 16)(*v)                       # noqa: E731
        return _lib.MaterialLawC(self.n, 0, self.k_ref, self.cp_ref, self.c_lo, a(self.x), a(self.kq), a(self.hks), a(self.ks2),
                                 a(self.th), a(self.c), a(self.hcs), a(self.cs2), a(self.H))

    def key(self):
        """every parameter of the law: a launch takes it by value, so a captured graph holds the law of its capture"""
        return (self.k_ref, self.cp_ref, self.c_lo, self.L, self.Ts, self.Tl) + tuple(
            tuple(v.tolist()) for v in (self.x, self.kq, self.ks, self.c, self.cs, self.th, self.H))


class _RatioLossPacks(LossPacks):
    """LossPacks under a MaterialLaw: every coefficient is written times robin_ratio (adi_matlaw_loss_update)"""

    def __init__(self, law, active, *args, **kwargs):
        self.law, self.active = law, active
        super().__init__(*args, **kwargs)

    def _launch(self, T, Tinf, k0, k1, full):
        if not self.active:                                   # no loss: the coefficients are the zeros they were built as
            return
        g, m = self.grid, self.mat
        t = _native_f64(g, T)
        Tinf = float(self.Tinf if Tinf is None else Tinf)
        check(lib.adi_matlaw_loss_update(ctypes.byref(self.law.as_c()), ctypes.byref(self.loss.as_c(Tinf)), Tinf, _p(t),
                                         _p(g.d_flags), _p(g.d_bricks), *g.layout.pd, g.dx, m.rho, m.cp, self._coeff, int(k0),
                                         int(k1), int(full), _stream()))


class NonlinearPacks:
    """What a step under a MaterialLaw runs with: `.mat` = law.material(rho), `.packs` = one ordinary
    precompute_coeff_packs_unified call with it (dir_value passed through law.theta; Neumann fluxes unchanged: a flux is energy),
    `.theta` the persistent device field the linear step runs on (the grid's layout; its pointer never changes) and
    `.theta_inf` = Theta(Tinf).  loss: a SurfaceLoss or None; the Robin coefficient of an exposed cell is stored as
    loss.h_of(T, face, Tinf) * law.robin_ratio(T, Tinf) * A / Ccell with Ccell from `.mat`, accumulated '-' face first, so the
    sweep's sink c (Theta - Theta_inf) carries exactly h(T) A (T - Tinf).  Pass it to the step as `material=` with `.packs`
    and `.mat`.
        begin(T, Tinf=None)        before the linear step: the coefficients from T (with a loss), then theta = Theta(T)
        recover(T_in, out)         after sweep 2: `out` holds theta*, and is overwritten with the new temperature
        rebuild(T, k_begin, k_end) after `grid.mask` changed on those planes of axis 2, as LossPacks.rebuild
        liquid_fraction(T)         f_eq(T) on the mask, 0 off it, as a DeviceField"""

    def __init__(self, grid, rho, law, Tinf, loss=None, dir_mask=None, dir_value=None, neumann=None, T=None):
        if not isinstance(law, MaterialLaw):
            raise TypeError("NonlinearPacks: law must be a MaterialLaw")
        if loss is not None and not isinstance(loss, SurfaceLoss):
            raise TypeError("NonlinearPacks: loss must be a SurfaceLoss or None")
        self.grid, self._law, self.loss, self.mat = grid, law, loss, law.material(rho)
        if dir_value is not None:
            dv = dir_value.get() if isinstance(dir_value, DeviceField) else dir_value
            dv = dv.cpu().numpy() if isinstance(dv, torch.Tensor) else dv
            dir_value = float(law.theta(float(dv))) if np.isscalar(dv) else law.theta(dv)
        self._lp = _RatioLossPacks(law, loss is not None, grid, self.mat, loss if loss is not None else SurfaceLoss(), Tinf, dir_mask=dir_mask,
                                   dir_value=dir_value, neumann=neumann)
        self.packs = self._lp.packs
        self.theta = grid.layout.empty(zero=True)
        self._set_ambient(Tinf)
        if T is not None:
            self.rebuild(T)

    @property
    def law(self):
        return self._law

    @law.setter
    def law(self, law):
        """another law with the same k_ref and cp_ref (`.mat` and `.packs` were built with them) and, where the packs hold
        Dirichlet values, the same k(T) (they are stored as Theta(value)); a captured graph is rebuilt"""
        if not isinstance(law, MaterialLaw):
            raise TypeError("NonlinearPacks: law must be a MaterialLaw")
        if (law.k_ref, law.cp_ref) != (self.mat.k, self.mat.cp):
            raise ValueError("NonlinearPacks: the new law has another k_ref or cp_ref; build new NonlinearPacks for it")
        old = self._law
        if self.packs[2].has_dir and not (np.array_equal(law.x, old.x) and np.array_equal(law.kq, old.kq)):
            raise ValueError("NonlinearPacks: the packs hold Dirichlet values as Theta(value) of the old k(T); build new "
                             "NonlinearPacks for the new law")
        self._law = self._lp.law = law
        self.theta_inf = float(law.theta(self.Tinf))

    def _set_ambient(self, Tinf):
        self.Tinf = self._lp.Tinf = float(Tinf)
        self.theta_inf = float(self.law.theta(self.Tinf))

    def begin(self, T, Tinf=None):
        """T: the step's input, a fp64 device field in the grid's layout.  Tinf: a new ambient (default: as it is)"""
        g = self.grid
        if Tinf is not None and float(Tinf) != self.Tinf:
            self._set_ambient(Tinf)
        t = _native_f64(g, T, "NonlinearPacks.begin: T must be a fp64 device field in the grid's layout")
        if self.loss is not None:
            self._lp.update(t)
        check(lib.adi_matlaw_theta(ctypes.byref(self.law.as_c()), _p(t), _p(self.theta), _p(g.d_flags), _p(g.d_bricks),
                                   *g.layout.pd, _stream()))
        return self.theta

    def recover(self, T_in, out, d_dir_mask=None):
        """adi_matlaw_recover: T_in the step's input, `out` theta* on entry and the new temperature on return (both fp64 device
        fields in the grid's layout); d_dir_mask: the Dirichlet cells (default: the packs')"""
        g = self.grid
        msg = "NonlinearPacks.recover: fp64 device fields in the grid's layout (the result is written in place)"
        a, b = _native_f64(g, T_in, msg), _native_f64(g, out, msg)
        dm = d_dir_mask if d_dir_mask is not None else (self.packs[2].d_dir_mask if self.packs[2].has_dir else None)
        check(lib.adi_matlaw_recover(ctypes.byref(self.law.as_c()), _p(a), _p(b), _p(g.d_flags), _p(g.d_bricks), _p(dm),
                                     *g.layout.pd, _stream()))
        return out

    def rebuild(self, T, k_begin=0, k_end=None):
        self._lp.rebuild(T, k_begin, k_end)
        return self.packs

    def liquid_fraction(self, T):
        g, law = self.grid, self.law
        t = _native_f64(g, T)
        if not law.L:
            return DeviceField(g.layout.empty(zero=True))
        f = ((t - law.Ts) / (law.Tl - law.Ts)).clamp_(0.0, 1.0)
        out = g.layout.empty(zero=True)
        out.copy_(torch.where(g.d_mask.to(torch.bool), f, torch.zeros_like(f)))
        return DeviceField(out)

    def graph_key(self):
        """what a captured graph holds: the laws by value, theta by pointer, the ambient by value"""
        return (self.law.key(), None if self.loss is None else self.loss.key(), self.Tinf, self.theta.data_ptr())
