"""adi3d_hip_cyl -- MI355X drop-in for the reference's cylindrical backend `adi3d_cyl_phi_v3`.

Operator surface of adi3d_cyl_phi_v3.py:33-68, :332-350:
    GridCyl, Material, Params, RobinR, ZBC, adi_step(Tn, grid, mat, prm, robin_r, zbc, S=None, theta=None)
plus adi_step_masked (quick_spiral_deposition_gif_v5.py:31-70).

Only the backward-Euler scheme is served: the reference's scheme="douglas" branch reads
uninitialised memory and omits the diffusivity, so there is nothing valid to match;
requesting it raises NotImplementedError instead of silently computing something else.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, Layout, to_device, _device, _stream, _p, _as_state, _wrap
from .heat_source import goldak_shape, goldak_q, _source_block
from .phase import PhaseChange
from .history import HistoryLevels
from .cyl_extras import CylPhaseField, CylThermalHistory
from .cyl_monitor import CylFieldMonitor
from .cyl_solid import CylSolidificationRecord

__all__ = ['StagedCylStepper', 'CylGoldakSource', 'GridCyl', 'Material', 'Params', 'RobinR', 'ZBC', 'adi_step', 'adi_step_masked', 'DeviceField', 'to_device',
           'CylPhaseField', 'CylThermalHistory', 'PhaseChange', 'HistoryLevels', 'CylFieldMonitor', 'CylSolidificationRecord']


class GridCyl:  # adi3d_cyl_phi_v3.py:33-43
    def __init__(self, nr, nphi, nz, dr, dphi, dz, R, R_in=0.0):
        """R_in: inner radius of an annular grid, r_i = R_in + (i + 1/2) dr.  The reference's own drivers and its only test
        pass it (quick_spiral_deposition_gif_v5.py:80, tests/test_spiral_vs_analytic.py:18) to a constructor that does not
        take it (TypeError at HEAD); here it is accepted and every formula is the reference's with r shifted."""
        self.nr = int(nr); self.nphi = int(nphi); self.nz = int(nz)
        self.dr = float(dr); self.dphi = float(dphi); self.dz = float(dz)
        self.R = float(R)
        self.R_in = float(R_in)
        self.r = self.R_in + (np.arange(self.nr, dtype=np.float64) + 0.5) * self.dr
        self.r_imh = self.r - 0.5 * self.dr
        self.r_iph = self.r + 0.5 * self.dr
        self.r_outer_face = self.r_iph[-1]
        self.layout = Layout(self.nr, self.nphi, self.nz, phys=(self.nr, self.nphi, self.nz))   # (no padded extents: the phi lines are periodic)
        self._plans = {}
        self._scratch = None

    @property
    def shape(self):
        return (self.nr, self.nphi, self.nz)

    def scratch(self):
        if self._scratch is None or self._scratch[0].device != _device():
            self._scratch = [self.layout.empty() for _ in range(2)]
        return self._scratch


class Material:  # :45-50
    def __init__(self, rho, cp, k):
        self.rho = float(rho); self.cp = float(cp); self.k = float(k)

    @property
    def alpha(self):
        return self.k / (self.rho * self.cp)


class Params:  # :52-54
    def __init__(self, dt, theta=0.5, scheme="be"):
        self.dt = float(dt); self.theta = float(theta); self.scheme = str(scheme).lower()


class RobinR:  # :56-58
    def __init__(self, h, T_inf):
        self.h = float(h); self.T_inf = float(T_inf)


class ZBC:  # :60-68
    def __init__(self, kind_bot='neumann0', kind_top='robin', h_bot=0.0, h_top=0.0,
                 T_inf_bot=20.0, T_inf_top=20.0, T_bot=20.0, T_top=20.0):
        self.kind_bot = kind_bot; self.kind_top = kind_top
        self.h_bot = float(h_bot); self.h_top = float(h_top)
        self.T_inf_bot = float(T_inf_bot); self.T_inf_top = float(T_inf_top)
        self.T_bot = float(T_bot); self.T_top = float(T_top)


class CylGoldakSource:
    """Goldak's double ellipsoid riding on the cylindrical grid, for the `S=` argument of adi_step / adi_step_masked and the
    `source=` argument of StagedCylStepper (include/adi_hip.h, "Moving heat source of the cylindrical step").
    power P [W], efficiency eta, a (transverse half-width), b (depth), c_f / c_r (front / rear length) [m], front fraction
    f_f (f_r = 2 - f_f).  The centre at time t is at radius r_c, angle phi0 + omega t (omega signed, rad/s) and height
    z0 + v_z t (from the bottom face; v_z = pitch |omega| / 2 pi: a helix, 0: a ring).  Offsets are Cartesian in the frame
    (tangent, radial, axial) at the centre, with delta = phi - phi_c and s = sign(omega) (+1 for 0):
        xi = s r sin(delta),  rho = r cos(delta) - r_c,  zeta = z - z_c
    depth='z' (the arc on top of a wall): E = 3 xi^2/c^2 + 3 rho^2/a^2 + 3 zeta^2/b^2; depth='r' (cladding on a cylinder
    face) swaps rho and zeta.  q = 6 sqrt(3) f eta P / (a b c pi^1.5) exp(-E) with (f, c) = (f_f, c_f) where xi >= 0, else
    (f_r, c_r); q = 0 where E > E_CUT = 40.  The ellipsoid is rigid: q integrates to 2 eta P over all space, to eta P over
    the half-space on one side of the centre plane normal to the depth axis.
    power, eta, f_f, r_c, phi0, omega, z0 and v_z may change between the runs of a StagedCylStepper without a new graph."""
    E_CUT = _lib.SOURCE_E_CUT

    def __init__(self, power, eta, a, b, c_f, c_r, f_f=0.6, *, r_c, phi0=0.0, omega=0.0, z0, v_z=0.0, depth='z'):
        self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f = power, eta, a, b, c_f, c_r, f_f
        self.r_c, self.phi0, self.omega, self.z0, self.v_z, self.depth = r_c, phi0, omega, z0, v_z, depth
        self.validate()

    def validate(self):
        """ValueError for any parameter adi_cyl_heat_source rejects (include/adi_hip.h); returns the twelve numbers"""
        vals = goldak_shape('CylGoldakSource', self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f,
                            more=(self.r_c, self.phi0, self.omega, self.z0, self.v_z))
        if vals[7] < 0:
            raise ValueError("CylGoldakSource: r_c < 0")
        if not isinstance(self.depth, str) or self.depth not in _lib.CYL_DEPTHS:
            raise ValueError("CylGoldakSource: depth must be 'z' (0) or 'r' (1)")
        return vals

    def as_c(self):
        v = self.validate()
        return _lib.CylHeatSource(*v, _lib.CYL_DEPTHS[self.depth], 0)

    def shape_key(self):
        """the support's shape (a change recaptures a stepper's graph)"""
        return (float(self.a), float(self.b), float(self.c_f), float(self.c_r), self.depth)

    def center(self, t):
        """(r_c, phi_c, z_c) at time t"""
        return (float(self.r_c), float(self.phi0) + float(self.omega) * float(t), float(self.z0) + float(self.v_z) * float(t))

    def q(self, r, phi, z, t):
        """q [W/m^3] at points (broadcast NumPy arrays: radius, angle, height) -- the host evaluator, the kernels' expression"""
        P, eta, a, b, cf, cr, ff, rc = self.validate()[:8]
        _, phic, zc = self.center(t)
        r, phi, z = (np.asarray(v, dtype=np.float64) for v in (r, phi, z))
        delta = phi - phic
        sgn = -1.0 if float(self.omega) < 0.0 else 1.0
        xi = sgn * (r * np.sin(delta))
        rho = r * np.cos(delta) - rc
        zeta = z - zc
        lrad, lax = (a, b) if self.depth == 'z' else (b, a)
        return goldak_q(xi, rho, zeta, xi >= 0.0, P, eta, lrad, lax, cf, cr, ff)

    def sample(self, grid, t, active=None):
        """q at the cell centres (r_i, (j+1/2) dphi, (k+1/2) dz) at time t: float64 array (nr, nphi, nz), 0 where `active`
        is False (NumPy: the ground truth the tests hold the kernels to)"""
        phi = (np.arange(grid.nphi, dtype=np.float64) + 0.5) * grid.dphi
        z = (np.arange(grid.nz, dtype=np.float64) + 0.5) * grid.dz
        q = np.broadcast_to(self.q(np.asarray(grid.r)[:, None, None], phi[None, :, None], z[None, None, :], t), grid.shape)
        return np.array(q) if active is None else np.where(np.asarray(active, dtype=bool), q, 0.0)

    def sample_device(self, grid, t, active=None):
        """the same on the device (adi_cyl_source_sample): a DeviceField"""
        out = grid.layout.empty(zero=True)
        d_act = None if active is None else grid.layout.to_layout(active, torch.uint8)
        check(lib.adi_cyl_source_sample(ctypes.byref(self.as_c()), grid.nr, grid.nphi, grid.nz, grid.layout.sx,
                                        grid.R_in, grid.dr, grid.dphi, grid.dz, float(t), _p(d_act), _p(out), _stream()))
        return DeviceField(out)

    def set_block(self, blk, t0, dt, n=0):
        check(lib.adi_cyl_source_set(_p(blk), ctypes.byref(self.as_c()), float(t0), float(dt), int(n), _stream()))


class _Plan:
    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            lib.adi_cyl_plan_destroy(self.handle)
        except Exception:
            pass


def _plan(grid, mat, dt, robin_r, zbc):
    if zbc.kind_bot not in _lib.ZBC_KINDS:
        raise ValueError("unknown zbc.kind_bot")     # adi3d_cyl_phi_v3.py:283
    if zbc.kind_top not in _lib.ZBC_KINDS:
        raise ValueError("unknown zbc.kind_top")     # :296
    key = (torch.cuda.current_device(), grid.dr, grid.dphi, grid.dz, getattr(grid, 'R_in', 0.0), mat.rho, mat.cp, mat.k, dt, robin_r.h,
           robin_r.T_inf, zbc.kind_bot, zbc.kind_top, zbc.h_bot, zbc.h_top, zbc.T_inf_bot, zbc.T_inf_top,
           zbc.T_bot, zbc.T_top)
    pl = grid._plans.get(key)
    if pl is None:
        _device()
        h = ctypes.c_void_p()
        check(lib.adi_cyl_plan_create_annular(grid.nr, grid.nphi, grid.nz, grid.layout.sx, grid.dr, grid.dphi, grid.dz,
                                              getattr(grid, 'R_in', 0.0), mat.rho, mat.cp, mat.k, dt, robin_r.h, robin_r.T_inf,
                                              _lib.ZBC_KINDS[zbc.kind_bot], _lib.ZBC_KINDS[zbc.kind_top], zbc.h_bot,
                                              zbc.h_top, zbc.T_inf_bot, zbc.T_inf_top, zbc.T_bot, zbc.T_top, ctypes.byref(h)))
        pl = _Plan(h)
        if len(grid._plans) > 16:      # drivers vary dt between segments; keep the cache bounded
            grid._plans.clear()
        grid._plans[key] = pl
    return pl


def _check_extras(who, grid, phase, history, monitor=None, solidification=None):
    """TypeError for an object of the wrong type, ValueError for one built for another grid: before the first launch"""
    if phase is not None and not isinstance(phase, CylPhaseField):
        raise TypeError("%s: phase must be a CylPhaseField" % who)
    if history is not None and not isinstance(history, CylThermalHistory):
        raise TypeError("%s: history must be a CylThermalHistory" % who)
    if monitor is not None and not isinstance(monitor, CylFieldMonitor):
        raise TypeError("%s: monitor must be a CylFieldMonitor" % who)
    if solidification is not None and not isinstance(solidification, CylSolidificationRecord):
        raise TypeError("%s: solidification must be a CylSolidificationRecord" % who)
    for name, obj in (('phase', phase), ('history', history), ('monitor', monitor), ('solidification', solidification)):
        if obj is not None and obj.grid is not grid:
            raise ValueError("%s: %s was built for another grid" % (who, name))


def _zbc_skips(zbc):
    """(skip_k0, skip_kN) of CylPhaseField.apply: the planes the z sweep pins"""
    return zbc.kind_bot == 'dirichlet', zbc.kind_top == 'dirichlet'


def _extras(x, out, prm, zbc, d_act, phase, history, monitor=None, solidification=None):
    """what follows the sweeps of a plain step x -> out: the latent-heat pass on out, the history's record of (x, out), the
    solidification record of (x, out), then the monitor's row from out"""
    if phase is not None:
        skip_k0, skip_kN = _zbc_skips(zbc)
        phase.apply(out, T_in=x, active=d_act, skip_k0=skip_k0, skip_kN=skip_kN)
    if history is not None:
        history._record_step(x, out, prm.dt, captured=False, d_act=d_act)
    if solidification is not None:                     # (no hot words: a caller of the plain step may activate cells)
        solidification._record_step(x, out, prm.dt, captured=False, d_act=d_act)
    if monitor is not None:
        monitor._record_step(x, out, prm.dt, captured=False, d_act=d_act)


def _run(Tn, grid, mat, prm, robin_r, zbc, S, active, T_void, T_inner, t=None, phase=None, history=None, monitor=None,
         solidification=None):
    # adi3d_cyl_phi_v3.py:335: `scheme = prm.scheme if prm.scheme in ('be', 'douglas') else 'be'` -- every string but
    # 'douglas' is backward Euler in the reference, and so it is here
    if prm.scheme == "douglas":
        raise NotImplementedError("adi3d_hip_cyl does not serve scheme='douglas': the reference's branch is numerically "
                                  "broken (reads uninitialised memory, omits alpha), so it has no valid oracle")
    _check_extras('adi_step' if active is None else 'adi_step_masked', grid, phase, history, monitor, solidification)
    src = S if isinstance(S, CylGoldakSource) else None
    if src is not None and t is None:
        raise ValueError("t (the step's start time) is required when S is a CylGoldakSource")
    x, kind = _as_state(Tn, grid)           # (a GridCyl has no mask to synchronise: the conversion alone)
    pl = _plan(grid, mat, prm.dt, robin_r, zbc)
    out = grid.layout.empty()
    d_act = None if active is None else grid.layout.to_layout(active, torch.uint8)
    if src is not None:           # q(t + dt/2) evaluated in the r sweep's load (adi_cyl_step_src)
        blk = _source_block(grid)
        src.set_block(blk, t, prm.dt)
        check(lib.adi_cyl_step_src(pl.handle, _p(blk), _p(x), _p(out), _p(d_act), float(T_void), float(T_inner), _stream()))
        _extras(x, out, prm, zbc, d_act, phase, history, monitor, solidification)
        return _wrap(out, kind)
    d_S = None if S is None else grid.layout.to_layout(S, torch.float64)
    check(lib.adi_cyl_step(pl.handle, _p(x), _p(out), None, None, _p(d_S), _p(d_act),
                           float(T_void), float(T_inner), _stream()))
    _extras(x, out, prm, zbc, d_act, phase, history, monitor, solidification)
    return _wrap(out, kind)


class StagedCylStepper:
    """adi_step (BE) with its arguments resolved once, for loops over a device-resident field and per-sweep timing:
    `events`: optional list of 4 torch.cuda.Event recorded on the launch stream before / between / after the r, phi
    and z sweeps (adi_cyl_sweep of the C ABI).
    source: a CylGoldakSource, evaluated in the r sweep's load at each step's mid-time from a device block (adi_cyl_sweep_src)
    whose step counter the z sweep advances; None issues the launches of a plain step.
    phase (a CylPhaseField of this grid): the latent-heat pass follows the z sweep, the planes a 'dirichlet' closure pins left
    alone.  history (a CylThermalHistory of this grid): the record of every step follows that, at the recorder's own clock; the
    record needs the step's input, so `run` then steps between two persistent fields instead of in place.  monitor (a
    CylFieldMonitor of this grid): its row of every step is the step's last launch, from the step's final field over every
    cell; it reads only the result, so it leaves `run` in place.  solidification (a CylSolidificationRecord of this grid): its
    record of every step follows the history's and needs the step's input as well, so `run` takes the two-field loop with it
    too; inside `run` -- no births, every input the previous result -- it is passed the hot words, which `run` seeds from its
    input.  None: the launches, results and graph key of before."""
    stage_names = ['sweep_r', 'sweep_phi', 'sweep_z_contig']
    stage_bytes_per_cell = [16.0, 16.0, 16.0]          # field in + field out per sweep

    def __init__(self, grid, mat, prm, robin_r, zbc, source=None, phase=None, history=None, monitor=None, solidification=None):
        if prm.scheme == "douglas":
            raise NotImplementedError("scheme='douglas' has no valid oracle (see adi_step)")
        if source is not None and not isinstance(source, CylGoldakSource):
            raise TypeError("StagedCylStepper: source must be a CylGoldakSource (pass a source field to adi_step)")
        _check_extras('StagedCylStepper', grid, phase, history, monitor, solidification)
        self.grid = grid
        self.dt = float(prm.dt)
        self.plan = _plan(grid, mat, prm.dt, robin_r, zbc)
        self.phase, self.history, self.monitor = phase, history, monitor
        self.solidification = solidification
        self._skips = _zbc_skips(zbc)
        self.source = source
        self.captures = 0
        if source is not None:
            source.validate()
            _source_block(self)                        # exists before any capture

    def _sweep(self, ax, a, b):
        if self.source is None:
            check(lib.adi_cyl_sweep(self.plan.handle, ax, _p(a), _p(b), None, None, 0.0, 0.0, _stream()))
        else:
            check(lib.adi_cyl_sweep_src(self.plan.handle, ax, _p(_source_block(self)), _p(a), _p(b), None, 0.0, 0.0,
                                        _stream()))

    def step(self, T, events=None, t=0.0):
        """r sweep T -> out, then the phi and z sweeps IN PLACE on out (every sweep kernel reads only the rows it writes):
        the input is untouched, as in the reference, and two of the three sweeps work on one field instead of two.
        t: the step's start time (the source, if any, at t + dt/2)"""
        g = self.grid
        if self.source is not None:
            self.source.set_block(_source_block(self), t, self.dt)
        out = g.layout.empty()
        self._step_into(g.layout.to_layout(T, torch.float64), out, events, captured=False)
        return DeviceField(out)

    def _step_into(self, x, out, events=None, captured=True):
        """the launches of one step x -> out (two fields): the sweeps, the latent-heat pass on out with newborn cells seeded
        from x, the records of (x, out) and their ticks.  captured: a graph may replay them and `run` keeps the recorders'
        clocks -- and the solidification record takes the hot words `run` has seeded"""
        self._sweeps(x, out, events)
        if self.phase is not None:
            self.phase.apply(out, T_in=x, skip_k0=self._skips[0], skip_kN=self._skips[1])
        if self.history is not None:
            self.history._record_step(x, out, self.dt, captured)
        if self.solidification is not None:
            self.solidification._record_step(x, out, self.dt, captured, hot=captured)
        if self.monitor is not None:
            self.monitor._record_step(x, out, self.dt, captured)

    def _sweeps(self, x, out, events):
        """the launches of one step: the r sweep x -> out, then the phi and z sweeps in place on out (out may be x)"""
        if events is not None:
            events[0].record()
        for ax in ((0, 1, 2) if self.grid.nphi > 1 else (0, 2)):
            self._sweep(ax, x if ax == 0 else out, out)
            if events is not None:
                events[ax + 1].record()
                if ax == 0 and self.grid.nphi == 1:
                    events[2].record()         # no phi sweep (phi_solve_spectral copies, :319-320): an empty interval

    def _step_inplace(self, x, events=None):
        """one step on x in place (native-layout device tensor), no allocation: what a HIP graph captures.
        events: as in step()"""
        self._sweeps(x, x, events)
        if self.phase is not None:                     # (nothing to seed from: `run` seeds the newborn cells before the loop)
            self.phase.apply(x, skip_k0=self._skips[0], skip_kN=self._skips[1])
        if self.monitor is not None:                   # (the row and the tick alone: `run` keeps the monitor's clock)
            self.monitor._record_step(None, x, self.dt, captured=True)

    def run(self, T, nsteps, graph=True, t0=0.0):
        """`nsteps` BE steps with the same plan on a device-resident field (the drivers' inner loops,
        quick_compare_layer_birth_robin_cyl_v3.py), returned as a new DeviceField.  The loop owns its field, so all three
        sweeps run IN PLACE: the working set is one field (134 MB at 128 x 256 x 512, inside the 256 MB Infinity Cache)
        instead of two -- 0.160 -> 0.144 ms per step.  The step is three kernels of ~45 us, at the edge of launch-bound: the
        launches of one step are captured once into a HIP graph and replayed.  Bit-identical to calling step() nsteps
        times.  graph=False: plain launches.
        t0: time at the start of the first step (a source's step i runs at t0 + i*dt + dt/2).  The source's block is written
        here, so its parameters as they are now hold for this run; a change of its support's shape recaptures.
        With a `phase` its launch follows the z sweep, in place as well.  With a `history` or a `solidification` the step's
        input must survive the step: see _run_recorded."""
        g = self.grid
        nsteps = int(nsteps)
        st = getattr(self, '_graph', None)
        key = (None if self.source is None else self.source.shape_key(),
               None if self.phase is None else self.phase.graph_key(),
               None if self.history is None else self.history.graph_key())
        if self.monitor is not None:
            key += (self.monitor.graph_key(),)
        if self.solidification is not None:
            key += (self.solidification.graph_key(),)
        recorded = self.history is not None or self.solidification is not None
        if st is None or st.get('key') != key:
            st = self._graph = dict(X=g.layout.empty(), Y=g.layout.empty() if recorded else None, g=None, key=key)
        X = st['X']
        X.copy_(g.layout.to_layout(T, torch.float64))
        if self.source is not None:
            self.source.set_block(_source_block(self), t0, self.dt)
        if recorded:
            return self._run_recorded(st, T, nsteps, graph, t0)
        if self.phase is not None:
            # the loop steps in place and so has no input to seed a newborn cell from: every cell the phase field has never
            # seen active is seeded here, from the field the first step starts with -- what step() would seed it from (the
            # planes the z sweep pins excepted, as there).  Looked for once per seed / restore of the phase field, not per run.
            if getattr(self, '_nan_free_at', None) != self.phase._edits:
                newborn = torch.isnan(self.phase.f)
                if self._skips[0]:
                    newborn[:, :, 0] = False
                if self._skips[1]:
                    newborn[:, :, -1] = False
                if bool(newborn.any().item()):
                    self.phase.seed(X, sel=newborn)
                self._nan_free_at = self.phase._edits
        mon = self.monitor
        if graph and nsteps >= 2 and st['g'] is None:
            stateful = [s for s in (self.phase, mon) if s is not None]
            held = [s.snapshot() for s in stateful]        # (the warm-up step would advance f, the monitor's log and block)
            self._step_inplace(X)                          # warm-up outside the capture (lazy module loads)
            X.copy_(g.layout.to_layout(T, torch.float64))
            for s, snap in zip(stateful, held):
                s.restore(snap)
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                self._step_inplace(X)
            st['g'] = cg
            self.captures += 1
            if self.source is not None:
                self.source.set_block(_source_block(self), t0, self.dt)   # (after the warm-up: the counter starts at 0)
        if mon is not None:
            mon.set_clock(self.dt)
        for _ in range(nsteps):
            if graph and st['g'] is not None:
                st['g'].replay()
            else:
                self._step_inplace(X)
        if mon is not None:
            mon.advance_clock(mon.t, self.dt, nsteps)
        out = g.layout.empty()
        out.copy_(X)
        return DeviceField(out)

    def _run_recorded(self, st, T, nsteps, graph, t0):
        """`run` with a history or a solidification record: a record needs the step's input, so the loop keeps two persistent
        fields -- r sweep X -> Y, phi and z in place on Y, the latent-heat pass on Y, the records of (X, Y) and their ticks, then
        the roles swap.  The launches of two steps (X -> Y -> X) are captured once and replayed, an odd last step is launched
        plainly: no per-step copy of the field, and the bits of step() called nsteps times.  Every recorder's block is set from
        the recorder's own clock; the solidification record's hot words are seeded from the run's input, after any warm-up."""
        g, sol = self.grid, self.solidification
        X, Y = st['X'], st['Y']
        clocked = [s for s in (self.history, sol, self.monitor) if s is not None]
        stateful = [s for s in (self.phase,) if s is not None] + clocked
        if graph and nsteps >= 2 and st['g'] is None:
            held = [s.snapshot() for s in stateful]        # (the warm-up steps would advance f, the state, the log and the clock)
            for s in clocked:
                s.set_clock(self.dt)
            self._step_into(X, Y); self._step_into(Y, X)   # warm-up outside the capture (lazy module loads)
            X.copy_(g.layout.to_layout(T, torch.float64))
            for s, snap in zip(stateful, held):
                s.restore(snap)
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                self._step_into(X, Y)
                self._step_into(Y, X)
            st['g'] = cg
            self.captures += 1
            if self.source is not None:
                self.source.set_block(_source_block(self), t0, self.dt)   # (after the warm-up: the counter starts at 0)
        for s in clocked:
            s.set_clock(self.dt)
        if sol is not None:
            sol.seed_hot(X)
        done = 0
        if graph and st['g'] is not None:
            for _ in range(nsteps // 2):
                st['g'].replay()
            done = 2 * (nsteps // 2)
        cur, oth = X, Y
        for _ in range(nsteps - done):
            self._step_into(cur, oth)
            cur, oth = oth, cur
        for s in clocked:
            s.advance_clock(s.t, self.dt, nsteps)
        out = g.layout.empty()
        out.copy_(cur)
        return DeviceField(out)


def adi_step(Tn, grid, mat, prm, robin_r, zbc, S=None, theta=None, t=None, phase=None, history=None, monitor=None,
             solidification=None):
    """adi3d_cyl_phi_v3.py:332-350 (BE branch: r -> phi -> z with theta = 1; `theta` is unused there too).
    S: a source field [W/m^3] of the grid's shape (the reference's argument), or a CylGoldakSource evaluated at t + dt/2 in
    the r sweep's load -- then `t`, the step's start time, is required.
    phase (a CylPhaseField of this grid): after the sweeps the latent-heat correction of the result, the planes a 'dirichlet'
    closure of `zbc` pins left alone.  history (a CylThermalHistory of this grid): then the record of the step Tn -> result at
    the recorder's own clock.  solidification (a CylSolidificationRecord of this grid): then its record of the same step, at its
    own clock.  monitor (a CylFieldMonitor of this grid): last, its row from the result.  All None: the launches and the bits of
    the call without them."""
    return _run(Tn, grid, mat, prm, robin_r, zbc, S, None, 0.0, 0.0, t, phase, history, monitor, solidification)


def adi_step_masked(Tn, grid, mat, prm, robin_outer, zbc, active, robin_inner=None, robin_void=None, S=None, t=None,
                    phase=None, history=None, monitor=None, solidification=None):
    """quick_spiral_deposition_gif_v5.py:31-70: void cells clamped to robin_void.T_inf before and after
    the step, inactive axis-row cells to robin_inner.T_inf; the clamps are fused into the r-sweep load
    and the z-sweep store.
    S: a CylGoldakSource (q(t + dt/2) added on active cells only; `t` required), or a source field added to the clamped
    field as adi_step(T_work, S=S) adds it.
    phase, history: as in adi_step, on the active cells; a cell that `active` holds for the first time is seeded from Tn (which
    equals the clamped field on every active cell), so an activation needs no call.  solidification, monitor: as in adi_step,
    over the active cells; the front's gradient takes a neighbour only where `active` holds it."""
    robin_inner = robin_inner or robin_outer
    robin_void = robin_void or robin_outer
    return _run(Tn, grid, mat, prm, robin_outer, zbc, S, active, robin_void.T_inf, robin_inner.T_inf, t, phase, history, monitor,
                solidification)
