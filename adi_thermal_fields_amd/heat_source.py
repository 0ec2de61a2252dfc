"""Goldak's double-ellipsoid heat source on the host: its one definition (`goldak_shape`, `goldak_q`), the moving source
`GoldakSource`, the step-averaged `ScanPath` with its frozen form `ScanPathSource`, which the library evaluates, and the device
block and workspace a moving source's owner keeps."""
import copy
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _device, _p, _stream


def goldak_shape(who, power, eta, a, b, c_f, c_r, f_f, more=()):
    """ValueError, its text prefixed by the class name `who`, for shape parameters of Goldak's double ellipsoid outside the
    ranges the library accepts (adi_heat_source, adi_cyl_heat_source: include/adi_hip.h); `more`: further parameters of the
    class that must be finite real numbers.  -> [power, eta, a, b, c_f, c_r, f_f, *more] as floats"""
    try:
        vals = [float(v) for v in (power, eta, a, b, c_f, c_r, f_f, *more)]
    except (TypeError, ValueError):
        raise ValueError("%s: parameters must be real numbers" % who)
    if not all(np.isfinite(v) for v in vals):
        raise ValueError("%s: non-finite parameter" % who)
    P, eta, a, b, cf, cr, ff = vals[:7]
    if P < 0:
        raise ValueError("%s: power < 0" % who)
    if not 0.0 <= eta <= 1.0:
        raise ValueError("%s: eta outside [0, 1]" % who)
    if min(a, b, cf, cr) <= 0:
        raise ValueError("%s: non-positive length (a, b, c_f, c_r must be > 0)" % who)
    if not 0.0 < ff < 2.0:
        raise ValueError("%s: f_f outside (0, 2)" % who)
    return vals


def goldak_amp(front, P, eta, a, b, c_f, c_r, f_f):
    """(amplitude 6 sqrt(3) f eta P / (a b c pi^1.5), c) with (f, c) = (f_f, c_f) where `front`, (2 - f_f, c_r) elsewhere"""
    f = np.where(front, f_f, 2.0 - f_f)
    cl = np.where(front, c_f, c_r)
    return (6.0 * np.sqrt(3.0) * f * eta * P) / (a * b * cl * np.pi ** 1.5), cl


def goldak_q(xi, y, z, front, P, eta, a, b, c_f, c_r, f_f):
    """q [W/m^3] of Goldak's double ellipsoid from the offsets to its centre in its own frame (broadcast NumPy arrays): xi
    along the travel direction, y across it (length a), z in depth (length b); `front`: where the offset lies ahead of the
    centre.  THE host evaluator, the same expression as the kernels': the exponent is summed as (travel + transverse) + depth,
    q = 0 where it exceeds E_CUT = 40 (ADI_SOURCE_E_CUT)."""
    amp, cl = goldak_amp(front, P, eta, a, b, c_f, c_r, f_f)
    E = (3.0 * (xi * xi) / (cl * cl) + 3.0 * (y * y) / (a * a)) + 3.0 * (z * z) / (b * b)
    with np.errstate(under='ignore'):
        return np.where(E <= _lib.SOURCE_E_CUT, amp * np.exp(-np.minimum(E, 745.0)), 0.0)


def _source_block(owner):
    """the device parameter block of a moving source (ADI_SOURCE_BLOCK_BYTES), one per grid / stepper / engine"""
    blk = getattr(owner, '_src_block', None)
    if blk is None or blk.device != _device():
        blk = owner._src_block = torch.zeros(_lib.SOURCE_BLOCK_BYTES, dtype=torch.uint8, device=_device())
    return blk


def _source_work(owner, dims, dx, src):
    """workspace of adi_source_lines0 on a box of `dims` = (nx, ny, nz) (lines longer than the in-register limit only; None
    otherwise), one per grid / stepper / engine, grown when a larger support needs more"""
    b = ctypes.c_size_t(0)
    check(lib.adi_source_workspace_bytes(ctypes.byref(src.as_c()), *dims, dx, ctypes.byref(b)))
    if b.value == 0:
        return None
    w = getattr(owner, '_src_work', None)
    if w is None or w.numel() < b.value or w.device != _device():
        w = owner._src_work = torch.empty(b.value, dtype=torch.uint8, device=_device())
    return w


class GoldakSource:
    """Goldak's double-ellipsoid heat source (Goldak, Chakravarti & Bibby 1984), axis-aligned, for the `S=` argument of
    adi_step_numba_coeff and the `source=` argument of StagedStepper.  power P [W], efficiency eta, a (transverse
    half-width), b (depth), c_f / c_r (front / rear length) [m], front fraction f_f (f_r = 2 - f_f).  The centre at time t
    is origin + travel_sign * velocity * t along travel_axis; depth_axis != travel_axis, the transverse axis is the third.
        q = 6 sqrt(3) f eta P / (a b c pi^1.5) exp(-3 xi^2/c^2 - 3 y^2/a^2 - 3 z^2/b^2),  (f, c) = (f_f, c_f) ahead of
        the centre (travel_sign*xi >= 0), (f_r, c_r) behind it; q = 0 where the exponent exceeds E_CUT = 40.
    Over all space q integrates to 2 eta P, over the half-space on one side of the centre plane normal to depth_axis to
    eta P: Goldak's normalisation for a centre on the surface.  The mask cuts the rest; nothing is renormalised.
    power, eta, f_f, origin and velocity may change between the runs of a StagedStepper without a new graph."""
    E_CUT = _lib.SOURCE_E_CUT

    def __init__(self, power, eta, a, b, c_f, c_r, f_f=0.6, origin=(0.0, 0.0, 0.0), velocity=0.0, travel_axis=1,
                 travel_sign=+1, depth_axis=2):
        self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f = power, eta, a, b, c_f, c_r, f_f
        self.origin, self.velocity = origin, velocity
        self.travel_axis, self.travel_sign, self.depth_axis = travel_axis, travel_sign, depth_axis
        self.validate()

    def validate(self):
        """ValueError for any parameter adi_heat_source rejects (include/adi_hip.h)"""
        vals = goldak_shape('GoldakSource', self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f,
                            more=(self.velocity,))
        try:
            org = tuple(float(v) for v in self.origin)
        except (TypeError, ValueError):
            raise ValueError("GoldakSource: origin must be three real numbers")
        if len(org) != 3:
            raise ValueError("GoldakSource: origin must have three coordinates")
        if not all(np.isfinite(v) for v in org):
            raise ValueError("GoldakSource: non-finite origin")
        if vals[7] < 0:
            raise ValueError("GoldakSource: velocity < 0 (the direction is travel_sign)")
        for name in ('travel_axis', 'depth_axis'):
            ax = getattr(self, name)
            if isinstance(ax, bool) or not isinstance(ax, (int, np.integer)) or not 0 <= ax <= 2:
                raise ValueError("GoldakSource: %s must be 0, 1 or 2" % name)
        if self.travel_axis == self.depth_axis:
            raise ValueError("GoldakSource: travel_axis == depth_axis")
        if self.travel_sign not in (1, -1) or isinstance(self.travel_sign, bool):
            raise ValueError("GoldakSource: travel_sign must be +1 or -1")
        return vals, org

    def as_c(self):
        (P, eta, a, b, cf, cr, ff, v), org = self.validate()
        return _lib.HeatSource(P, eta, a, b, cf, cr, ff, (ctypes.c_double * 3)(*org), v, int(self.travel_axis),
                               int(self.travel_sign), int(self.depth_axis), 0)

    def shape_key(self):
        """what the launch box of the moving-source kernel depends on (a change recaptures a stepper's graph)"""
        return (float(self.a), float(self.b), float(self.c_f), float(self.c_r), int(self.travel_axis),
                int(self.travel_sign), int(self.depth_axis))

    def center(self, t):
        c = np.array([float(v) for v in self.origin], dtype=np.float64)
        c[self.travel_axis] = c[self.travel_axis] + (float(self.travel_sign) * float(self.velocity)) * float(t)
        return c

    def q(self, x0, x1, x2, t):
        """q [W/m^3] at points (broadcast NumPy arrays, metres) -- the host evaluator, same expression as the kernels'"""
        (P, eta, a, b, cf, cr, ff, _), _ = self.validate()
        c = self.center(t)
        o = (np.asarray(x0, dtype=np.float64) - c[0], np.asarray(x1, dtype=np.float64) - c[1],
             np.asarray(x2, dtype=np.float64) - c[2])
        ta, da = self.travel_axis, self.depth_axis
        xi, y, z = o[ta], o[3 - ta - da], o[da]
        return goldak_q(xi, y, z, float(self.travel_sign) * xi >= 0.0, P, eta, a, b, cf, cr, ff)

    def sample(self, grid, t):
        """q at the cell centres ((i+1/2)dx, (j+1/2)dx, (k+1/2)dx) at time t: float64 array of the grid's shape, 0 off the
        mask (NumPy: the ground truth the tests hold the kernels to)"""
        dx = float(grid.dx)
        x = [(np.arange(n, dtype=np.float64) + 0.5) * dx for n in (grid.nx, grid.ny, grid.nz)]
        q = self.q(x[0][:, None, None], x[1][None, :, None], x[2][None, None, :], t)
        q = np.broadcast_to(q, (grid.nx, grid.ny, grid.nz))
        return np.where(np.asarray(grid.mask, dtype=bool), q, 0.0)

    def sample_device(self, grid, t):
        """the same on the device (adi_source_sample): a DeviceField"""
        out = grid.layout.empty()
        check(lib.adi_source_sample(ctypes.byref(self.as_c()), _p(grid.d_flags), *grid.layout.pd, grid.dx, float(t),
                                    _p(out), _stream()))
        return DeviceField(out)

    def set_block(self, blk, t0, dt, n=0):
        check(lib.adi_source_set(_p(blk), ctypes.byref(self.as_c()), float(t0), float(dt), int(n), _stream()))


_erf = np.frompyfunc(math.erf, 1, 1)


class ScanPath:
    """Goldak's double ellipsoid driven along a path of straight segments (README, "Scan paths"): the HOST definition
    of its step-averaged heat input.  A step takes it as a source field, adi_step_numba_coeff(..., S=path.sample_step(grid, t,
    dt)); a path is not accepted as `S=` itself or as `source=` of a StagedStepper.  `path.on_device()` freezes it into a
    ScanPathSource, whose `sample_step_device` evaluates the same field on the device (no NumPy erf, nothing over PCIe).
    Shape as GoldakSource: efficiency eta, a (half-width across the leg), b (depth), c_f / c_r (front / rear length) [m], front
    fraction f_f; depth along depth_axis, the other two axes in increasing order are the in-plane axes (u, v).  `power` [W] is
    the default of line_to.
    The path starts at `start` (metres) at time t_start; line_to adds a straight leg at constant speed (power 0: a jump with
    the beam off), dwell a stationary segment.  Segment k is active on [t_k, t_{k+1}).
    The source of a step [t, t + dt] is q_step: the exact time average of the moving source over the step, summed over the
    segments the step overlaps -- not a sample at mid-step, so a step may cross any number of legs, corners and jumps.
    The cuts bound xi and (y, z) separately: the support around the centre is a box in the leg's frame."""
    E_CUT = _lib.SOURCE_E_CUT
    DELTA_MIN = 1e-3          # travel of a piece over min(c_f, c_r) below which q_step uses Simpson's rule instead of erf

    def __init__(self, eta, a, b, c_f, c_r, f_f=0.6, depth_axis=2, power=0.0, start=(0.0, 0.0, 0.0), t_start=0.0):
        self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f = eta, a, b, c_f, c_r, f_f
        self.depth_axis, self.power = depth_axis, power
        self.validate()
        self._pos = self._point(start, 'start')
        self.start = self._pos
        self.t_start = self._num(t_start, 't_start')
        self._t_end = self.t_start
        self._seg = []            # (t_begin, p0 (3), p1 (3), (d_u, d_v), speed, power)

    @staticmethod
    def _num(v, name, positive=False, nonneg=False):
        try:
            x = float(v)
        except (TypeError, ValueError):
            raise ValueError("ScanPath: %s must be a real number" % name)
        if not np.isfinite(x):
            raise ValueError("ScanPath: non-finite %s" % name)
        if (positive and x <= 0) or (nonneg and x < 0):
            raise ValueError("ScanPath: %s must be %s" % (name, '> 0' if positive else '>= 0'))
        return x

    @classmethod
    def _point(cls, p, name):
        try:
            q = tuple(float(v) for v in p)
        except (TypeError, ValueError):
            raise ValueError("ScanPath: %s must be three real numbers" % name)
        if len(q) != 3:
            raise ValueError("ScanPath: %s must have three coordinates" % name)
        if not all(np.isfinite(v) for v in q):
            raise ValueError("ScanPath: non-finite %s" % name)
        return q

    def validate(self):
        """ValueError for a shape parameter out of range (the ranges of GoldakSource)"""
        vals = goldak_shape('ScanPath', self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f)
        ax = self.depth_axis
        if isinstance(ax, bool) or not isinstance(ax, (int, np.integer)) or not 0 <= ax <= 2:
            raise ValueError("ScanPath: depth_axis must be 0, 1 or 2")
        return vals[1:]

    @property
    def axes(self):
        """(u, v): the in-plane axes"""
        da = int(self.depth_axis)
        return (1 if da == 0 else 0), (1 if da == 2 else 2)

    def _add(self, p1, d, speed, power, duration):
        self._seg.append((self._t_end, self._pos, p1, d, speed, power))
        self._pos = p1
        self._t_end = self._t_end + duration
        return self

    def line_to(self, point, speed, power=None):
        """a straight leg from the current point to `point` at `speed` [m/s]; power None: the path's default, 0: a jump.  A leg
        with power keeps the depth coordinate; a jump may move anywhere (its time is its length in space over `speed`)."""
        p1 = self._point(point, 'point')
        speed = self._num(speed, 'speed', positive=True)
        P = self._num(self.power if power is None else power, 'power', nonneg=True)
        u, v = self.axes
        du, dv, dz = p1[u] - self._pos[u], p1[v] - self._pos[v], p1[self.depth_axis] - self._pos[self.depth_axis]
        plane = math.hypot(du, dv)
        length = math.hypot(plane, dz)
        if length == 0.0:
            raise ValueError("ScanPath.line_to: a leg of zero length (use dwell)")
        if P > 0 and dz != 0.0:
            raise ValueError("ScanPath.line_to: a leg with power must keep the depth coordinate")
        duration = length / speed
        if not (np.isfinite(duration) and self._t_end + duration > self._t_end):
            raise ValueError("ScanPath.line_to: the leg takes no time at this speed")
        if plane > 0.0:
            d, vel = (du / plane, dv / plane), plane / duration if dz != 0.0 else speed
            n = math.hypot(*d)
            d = (d[0] / n, d[1] / n)
        else:
            d, vel = (1.0, 0.0), 0.0
        return self._add(p1, d, vel, P, duration)

    def dwell(self, duration, power=0.0):
        """a stationary segment; with power the ellipsoid keeps the direction of the leg before it ((1, 0) at the start)"""
        duration = self._num(duration, 'duration', positive=True)
        P = self._num(power, 'power', nonneg=True)
        if not self._t_end + duration > self._t_end:
            raise ValueError("ScanPath.dwell: the dwell takes no time")
        d = self._seg[-1][3] if self._seg else (1.0, 0.0)
        return self._add(self._pos, d, 0.0, P, duration)

    @classmethod
    def raster(cls, lo, hi, hatch, speed, power, angle_deg=0.0, bidirectional=True, jump_speed=None, depth=0.0, t_start=0.0,
               **shape):
        """a hatch over the in-plane rectangle lo = (u_lo, v_lo) .. hi = (u_hi, v_hi) at depth coordinate `depth`: parallel
        tracks along (cos, sin)(angle_deg) spaced `hatch` apart along the normal (-sin, cos), the first through the corner with
        the lowest normal coordinate, each clipped to the rectangle.  bidirectional: every other track runs backwards and a
        jump (power 0, jump_speed, default `speed`) joins the end of a track to the start of the next; otherwise every track
        runs forwards and the jump flies back."""
        ulo, vlo = (cls._num(x, 'lo') for x in lo)
        uhi, vhi = (cls._num(x, 'hi') for x in hi)
        hatch = cls._num(hatch, 'hatch', positive=True)
        depth = cls._num(depth, 'depth')
        ang = math.radians(cls._num(angle_deg, 'angle_deg'))
        if not (uhi > ulo and vhi > vlo):
            raise ValueError("ScanPath.raster: empty rectangle")
        jump_speed = speed if jump_speed is None else jump_speed
        c, s = math.cos(ang), math.sin(ang)
        if abs(c) < 1e-15:
            c = 0.0
        if abs(s) < 1e-15:
            s = 0.0
        corners = [(ulo, vlo), (uhi, vlo), (uhi, vhi), (ulo, vhi)]
        sn = [-pu * s + pv * c for pu, pv in corners]
        n_tracks = int(math.floor((max(sn) - min(sn)) / hatch + 1e-9)) + 1
        tracks = []
        for i in range(n_tracks):
            off = min(sn) + i * hatch
            # the line {off*n + l*t}: clip l to the rectangle (slab method)
            ou, ov = -off * s, off * c
            l0, l1 = -np.inf, np.inf
            ok = True
            for o, dcomp, a0, a1 in ((ou, c, ulo, uhi), (ov, s, vlo, vhi)):
                if dcomp == 0.0:
                    ok = ok and (a0 - 1e-12 * max(1.0, abs(a0)) <= o <= a1 + 1e-12 * max(1.0, abs(a1)))
                else:
                    la, lb = (a0 - o) / dcomp, (a1 - o) / dcomp
                    l0, l1 = max(l0, min(la, lb)), min(l1, max(la, lb))
            if ok and l1 - l0 > 1e-9 * hatch:
                tracks.append(((ou + l0 * c, ov + l0 * s), (ou + l1 * c, ov + l1 * s)))
        if not tracks:
            raise ValueError("ScanPath.raster: no track fits the rectangle")
        da = shape.get('depth_axis', 2)
        u, v = (1 if da == 0 else 0), (1 if da == 2 else 2)

        def pt(q):
            p = [0.0, 0.0, 0.0]
            p[u], p[v], p[da] = q[0], q[1], depth
            return tuple(p)
        path = None
        for i, (q0, q1) in enumerate(tracks):
            if bidirectional and i % 2 == 1:
                q0, q1 = q1, q0
            if path is None:
                path = cls(power=power, start=pt(q0), t_start=t_start, **shape)
            else:
                path.line_to(pt(q0), jump_speed, power=0.0)
            path.line_to(pt(q1), speed)
        return path

    def on_device(self):
        """the path as it is now, frozen for the device: a ScanPathSource"""
        return ScanPathSource(self)

    # ---- plain readings
    @property
    def t_end(self):
        return self._t_end

    @property
    def n_segments(self):
        return len(self._seg)

    def _t_next(self, k):
        return self._seg[k + 1][0] if k + 1 < len(self._seg) else self._t_end

    def _index(self, t):
        """segment active at time t (a boundary belongs to the later segment); None outside [t_start, t_end)"""
        if not self._seg or t < self.t_start or t >= self._t_end:
            return None
        return int(np.searchsorted([s[0] for s in self._seg], t, side='right')) - 1

    def center(self, t):
        """the centre at time t: the start before t_start, the last point from t_end on"""
        t = float(t)
        k = self._index(t)
        if k is None:
            return np.array(self.start if (t < self.t_start or not self._seg) else self._pos, dtype=np.float64)
        tb, p0, p1 = self._seg[k][:3]
        lam = (t - tb) / (self._t_next(k) - tb)
        return np.array([a + (b - a) * lam for a, b in zip(p0, p1)], dtype=np.float64)

    def power_at(self, t):
        k = self._index(float(t))
        return 0.0 if k is None else self._seg[k][5]

    def table(self):
        """the segments as a float64 array (K, 8): t_begin, start point p[3], in-plane unit direction d[2], speed, power"""
        if not self._seg:
            raise ValueError("ScanPath: the path has no segment")
        return np.array([[tb, p0[0], p0[1], p0[2], d[0], d[1], vel, P] for tb, p0, _, d, vel, P in self._seg], dtype=np.float64)

    # ---- the definition
    def _piece(self, k, t, t1):
        """(ta, tb, w): the piece of segment k inside [t, t1] as times since its start and its length; None if it deposits
        nothing"""
        tb, _, _, _, _, P = self._seg[k]
        if not P > 0.0:
            return None
        tau0 = max(t, tb)
        tau1 = min(t1, self._t_next(k))
        if not tau1 > tau0:
            return None
        return tau0 - tb, tau1 - tb, tau1 - tau0

    def _qi(self, P, xi, Et):
        """the instantaneous double ellipsoid at along-leg offset xi, Et the exponent of the other two axes (no cut of its own)"""
        eta, a, b, cf, cr, ff = self.validate()
        amp, cl = goldak_amp(xi >= 0.0, P, eta, a, b, cf, cr, ff)
        E = 3.0 * (xi * xi) / (cl * cl) + Et
        with np.errstate(under='ignore'):
            return amp * np.exp(-E)

    def _qbar(self, k, x0, x1, x2, t, dt, branch=None):
        """qbar_k at points (broadcast arrays): the time average over [t, t + dt] of the moving source during its overlap with
        segment k.  branch: None -- the definition; 'erf' / 'simpson' force one of the two forms (tests)."""
        eta, a, b, cf, cr, ff = self.validate()
        shape = np.broadcast(x0, x1, x2).shape
        out = np.zeros(shape, dtype=np.float64)
        pc = self._piece(k, t, t + dt)
        if pc is None:
            return out
        ta, tb, w = pc
        _, p0, _, d, vel, P = self._seg[k]
        u, v = self.axes
        o = (x0 - p0[0], x1 - p0[1], x2 - p0[2])
        ou, ov, z = o[u], o[v], o[self.depth_axis]
        xi0 = ou * d[0] + ov * d[1]
        y = ov * d[0] - ou * d[1]
        xia = xi0 - vel * ta
        xib = xi0 - vel * tb
        Et = 3.0 * (y * y) / (a * a) + 3.0 * (z * z) / (b * b)
        R = np.sqrt(self.E_CUT / 3.0)
        ok = np.broadcast_to((Et <= self.E_CUT) & (xib <= R * cf) & (xia >= -(R * cr)), shape)
        if not ok.any():
            return out
        xi0, xia, xib, Et = (np.broadcast_to(q, shape)[ok] for q in (xi0, xia, xib, Et))
        travel = vel * w
        delta = travel / min(cf, cr)
        if branch == 'erf' or (branch is None and delta >= self.DELTA_MIN):
            s3 = np.sqrt(3.0)
            Ff = _erf(s3 * np.maximum(xia, 0.0) / cf).astype(np.float64) - _erf(s3 * np.maximum(xib, 0.0) / cf).astype(np.float64)
            Fr = _erf(s3 * np.minimum(xia, 0.0) / cr).astype(np.float64) - _erf(s3 * np.minimum(xib, 0.0) / cr).astype(np.float64)
            brace = ff * Ff + (2.0 - ff) * Fr
            amp = (3.0 * eta * P) / (np.pi * a * b * vel * dt)
            with np.errstate(under='ignore'):
                val = (amp * np.exp(-Et)) * brace
        elif travel == 0.0:
            val = (w / dt) * self._qi(P, xia, Et)
        else:
            xim = xi0 - vel * (0.5 * (ta + tb))
            qs = (self._qi(P, xia, Et) + 4.0 * self._qi(P, xim, Et)) + self._qi(P, xib, Et)
            val = (w / dt) * (qs / 6.0)
        out[ok] = val
        return out

    def q_step(self, x0, x1, x2, t, dt):
        """the source of the step [t, t + dt] in W/m^3 at points (broadcast NumPy arrays, metres): the sum over the segments, in
        ascending order, of their time averages: one fp64 operation per line"""
        t, dt = float(t), self._num(dt, 'dt', positive=True)
        x0, x1, x2 = (np.asarray(x, dtype=np.float64) for x in (x0, x1, x2))
        q = np.zeros(np.broadcast(x0, x1, x2).shape, dtype=np.float64)
        for k in range(len(self._seg)):
            if self._piece(k, t, t + dt) is not None:
                q += self._qbar(k, x0, x1, x2, t, dt)
        return q

    def _index_box(self, k, pc, n, dx):
        """slices of the cells of an n[0] x n[1] x n[2] grid whose centres can lie in the support of piece pc of segment k: the
        support reaches R hypot(max(c_f, c_r), a) from the centre in the plane and R b in depth (the cuts of _qbar)"""
        eta, a, b, cf, cr, ff = self.validate()
        R = np.sqrt(self.E_CUT / 3.0)
        _, p0, _, d, vel, _ = self._seg[k]
        u, v = self.axes
        dirs = {u: d[0], v: d[1], int(self.depth_axis): 0.0}
        sl = []
        for ax in range(3):
            m = (R * b if ax == self.depth_axis else R * math.hypot(max(cf, cr), a)) * (1.0 + 1e-9)
            ca, cb = p0[ax] + dirs[ax] * (vel * pc[0]), p0[ax] + dirs[ax] * (vel * pc[1])
            lo = int(min(max(math.floor((min(ca, cb) - m) / dx - 0.5), 0), n[ax]))
            hi = int(min(max(math.ceil((max(ca, cb) + m) / dx - 0.5) + 1, 0), n[ax]))
            sl.append(slice(lo, max(hi, lo)))
        return tuple(sl)

    def sample_step(self, grid, t, dt):
        """q_step at the cell centres ((i+1/2)dx, (j+1/2)dx, (k+1/2)dx): float64 array of the grid's shape, 0 off the mask: the
        source field of the step, for `S=`.  Every segment is evaluated on the index box of its support only (the cells outside
        it get exactly 0 from q_step), so the temporaries are of the size of the support, not of the grid."""
        t, dt = float(t), self._num(dt, 'dt', positive=True)
        dx = float(grid.dx)
        n = (grid.nx, grid.ny, grid.nz)
        x = [(np.arange(m, dtype=np.float64) + 0.5) * dx for m in n]
        q = np.zeros(n, dtype=np.float64)
        for k in range(len(self._seg)):
            pc = self._piece(k, t, t + dt)
            if pc is None:
                continue
            si, sj, sk = self._index_box(k, pc, n, dx)
            q[si, sj, sk] += self._qbar(k, x[0][si, None, None], x[1][None, sj, None], x[2][None, None, sk], t, dt)
        return np.where(np.asarray(grid.mask, dtype=bool), q, 0.0)


class ScanPathSource:
    """A ScanPath frozen for the device (`ScanPathSource(path)`, `path.on_device()`).  It snapshots the path's segment table,
    t_start, t_end, shape and depth_axis: later line_to / dwell calls on `path` do not reach it, and nothing of it can be changed
    (another power or path: make a new one).  It owns one device tensor, the table (K x 8 fp64 as ScanPath.table(), then
    t_end), allocated here on the current device and never written again.  ValueError for a path without segments.
    `sample_step_device(grid, t, dt)` is q_step of the step [t, t + dt] evaluated by the device (adi_scan_sample: include/adi_hip.h,
    "Scan path"), a DeviceField for the `S=` argument of adi_step_numba_coeff; `sample_step_host` the same code run by the library
    on the CPU; `sample_step` the NumPy definition of the snapshot.  Like a ScanPath it is not itself accepted as `S=` or as
    `source=` of a StagedStepper."""

    def __init__(self, path):
        if not isinstance(path, ScanPath):
            raise TypeError("ScanPathSource: a ScanPath is needed, got %s" % type(path).__name__)
        tab = path.table()                                   # (ValueError: the path has no segment)
        eta, a, b, cf, cr, ff = path.validate()
        snap = copy.copy(path)
        snap._seg = list(path._seg)
        self._path = snap                                    # the host definition of this very snapshot
        self.K = int(tab.shape[0])
        self.t_start, self.t_end = float(path.t_start), float(path.t_end)
        self.shape_params = (eta, a, b, cf, cr, ff)
        self.depth_axis = int(path.depth_axis)
        self._h_table = np.ascontiguousarray(np.concatenate([tab.ravel(), [self.t_end]]), dtype=np.float64)
        self._h_table.setflags(write=False)
        self._c_shape = _lib.ScanShape(eta, a, b, cf, cr, ff, self.depth_axis, 0)
        one = np.empty(1)                                    # (the library's own checks of the table, before any launch)
        check(lib.adi_scan_sample_host(*self._path_args(self._h_table.ctypes.data), None, 1, 1, 1, 1.0, self.t_start, 1.0,
                                       one.ctypes.data))
        dev = _device() if torch.cuda.is_available() else torch.device('cpu')   # (no GPU: the host evaluators only)
        self.d_table = torch.from_numpy(self._h_table.copy()).to(dev)

    def table(self):
        """the snapshot's segments, (K, 8) float64, read-only"""
        return self._h_table[:-1].reshape(self.K, _lib.SCAN_TABLE_COLS)

    def graph_key(self):
        """what a launch holds of the source: the table's address, K and the shape"""
        return (self.d_table.data_ptr(), self.K, self.shape_params + (self.depth_axis,))

    def _path_args(self, table):
        return ctypes.byref(self._c_shape), table, self.K, self.t_end

    # ---- the host definition
    def sample_step(self, grid, t, dt):
        """ScanPath.sample_step of the snapshot (NumPy: the ground truth the tests hold the kernels to)"""
        return self._path.sample_step(grid, t, dt)

    def sample_step_host(self, grid, t, dt):
        """the library's evaluator on the CPU (adi_scan_sample_host, no GPU needed): q_step at the cell centres of anything with
        nx, ny, nz, dx and mask, 0 off the mask"""
        n = (int(grid.nx), int(grid.ny), int(grid.nz))
        mask = np.ascontiguousarray(np.asarray(grid.mask, dtype=bool), dtype=np.uint8)
        if mask.shape != n:
            raise ValueError("sample_step_host: the mask has shape %s, the grid %s" % (mask.shape, n))
        out = np.empty(n, dtype=np.float64)
        check(lib.adi_scan_sample_host(*self._path_args(self._h_table.ctypes.data), mask.ctypes.data, *n, float(grid.dx),
                                       float(t), float(dt), out.ctypes.data))
        return out

    # ---- the device
    def sample_step_device(self, grid, t, dt):
        """q_step of the step [t, t + dt] at the cell centres, evaluated on the device (adi_scan_sample): a DeviceField"""
        out = grid.layout.empty()
        check(lib.adi_scan_sample(*self._path_args(_p(self.d_table)), _p(grid.d_flags), *grid.layout.pd, grid.dx, float(t),
                                  float(dt), _p(out), _stream()))
        return DeviceField(out)
