"""Latent heat and thermal history of the cylindrical step: the liquid fraction of a GridCyl, `CylPhaseField`, and the recorder of
peak temperature, cooling time and melt pool, `CylThermalHistory` (include/adi_hip.h, "Latent heat and thermal history of the
cylindrical step").  The laws are the Cartesian ones -- PhaseChange.correct, ThermalHistory.record_reference
and ThermalHistory.seed_reference stay the definitions, the cylindrical definitions below are compositions of them -- and the
conventions are the cylindrical backend's: `active` is an optional per-call array (None: every cell), there are no flags, no
bricks and no mask version, and a NaN in the state marks a cell that has never been seen active: the first pass that sees it
active seeds it from the step's input, so a birth needs no call."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _device, _native_f64, _p, _stream
from .phase import PhaseChange
from .history import HistoryLevels, ThermalHistory, _StepRecorder


def _active_arg(grid, active):
    """`active` (None / array / tensor of the grid's shape) as a uint8 device tensor in the grid's layout, or None"""
    return None if active is None else grid.layout.to_layout(active, torch.uint8)


def _seeded_state(grid, d_act, value):
    """a flat fp64 buffer of the grid's layout: `value` on the cells of d_act (None: all), NaN elsewhere"""
    L = grid.layout
    flat = torch.full((L.numel_padded,), float('nan') if d_act is not None else value, dtype=torch.float64, device=_device())
    if d_act is not None:
        flat.as_strided(L.shape, L.strides)[d_act != 0] = value
    return flat


def _decode_log(rec):
    """the cylindrical log of a recorder (`d_log`, `capacity`, `slot`, `_times`, `grid`) over its recorded steps: what
    CylThermalHistory.melt_pool and CylSolidificationRecord.front return"""
    slot = rec.slot
    n = min(slot, rec.capacity)
    rows = rec.d_log.cpu().numpy().reshape(rec.capacity + 1, _lib.CYL_HISTORY_LOG_INTS)[:n]
    cells, lo, hi = rows[:, 0].copy(), rows[:, 1:4].copy(), rows[:, 4:7].copy()
    sum_i = np.ascontiguousarray(rows[:, 8:10]).view(np.int64)[:, 0].copy()
    g = rec.grid
    volume = CylThermalHistory.pool_volume(g, cells, sum_i)
    span = np.where((cells > 0)[:, None], hi.astype(np.int64) - lo.astype(np.int64) + 1, 0)
    return dict(t=np.asarray(rec._times[:n], dtype=np.float64), cells=cells, lo=lo, hi=hi, sum_i=sum_i, volume=volume,
                extent_r=span[:, 0] * g.dr, extent_z=span[:, 2] * g.dz, dropped=max(0, slot - rec.capacity))


class CylPhaseField:
    """The liquid fraction of a GridCyl under a PhaseChange law, on the device: `f` (fp64, the grid's layout), NaN on a cell that
    has never been seen active, 0, 1 or in between otherwise.  T (optional): f = f_eq(T) on the cells of `active` (None: all)
    and NaN elsewhere; without T, f is 0 on them.  The buffer lives as long as the object, so a StagedCylStepper's graph holds
    its pointer.  A cell of a plane that `apply` skips (skip_k0 / skip_kN: the z sweep's Dirichlet rows) is never written, not
    even to seed it: a cell born on such a plane keeps its NaN for as long as the plane is pinned and reads as 0 in
    `liquid_fraction`, also where the plane is pinned above the liquidus.
        apply(T_star, T_in=None, active=None, skip_k0=False, skip_kN=False)   the correction, T_star and f in place: one launch
        seed(T, sel=None, active=None)     f = f_eq(T) on the active cells `sel` selects (None: all of them), NaN off `active`
        liquid_fraction                    a copy with NaN replaced by 0
        snapshot() / restore(s), graph_key()
    `apply_reference` is the definition, adi_cyl_phase_apply the same operations on the device and adi_cyl_phase_apply_host on
    the CPU."""

    def __init__(self, grid, mat, law, T=None, active=None):
        if not isinstance(law, PhaseChange):
            raise TypeError("CylPhaseField: law must be a PhaseChange")
        law.constants(mat.cp)
        self.grid, self.mat, self.law = grid, mat, law
        L = grid.layout
        d_act = _active_arg(grid, active)
        self._flat = _seeded_state(grid, d_act, 0.0)
        self.f = self._flat.as_strided(L.shape, L.strides)
        self._edits = 0              # seeds and restores so far (a stepper's in-place loop looks for NaN cells again after one)
        if T is not None:
            self.seed(T, active=d_act)

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def skip_planes(shape, skip_k0=False, skip_kN=False):
        """the cells of the planes k = 0 / k = nz - 1 an `apply` with these flags leaves alone, as a bool array"""
        skip = np.zeros(shape, dtype=bool)
        if skip_k0:
            skip[:, :, 0] = True
        if skip_kN:
            skip[:, :, -1] = True
        return skip

    @staticmethod
    def apply_reference(T_star, f, T_in, active, skip, law, cp):
        """(T, f) after the pass on the step's result T_star from the liquid fraction f: THE DEFINITION.  active: bool array
        (None: every cell); skip: the cells of the skipped Dirichlet planes (None: none; `skip_planes`); T_in: the step's input
        (None: nothing is seeded).  An active cell off the skipped planes whose f is NaN is a newborn and takes
        f = law.f_eq(T_in); then law.correct runs with mask=active and dir_mask=skip.  A cell of a skipped plane is never
        written, so a newborn there keeps its NaN until a pass that does not skip it.  Inactive cells keep their NaN."""
        Tst = np.asarray(T_star, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64)
        act = np.ones(Tst.shape, dtype=bool) if active is None else np.asarray(active, dtype=bool)
        skip = np.zeros(Tst.shape, dtype=bool) if skip is None else np.asarray(skip, dtype=bool)
        if T_in is not None:
            f = np.where(act & ~skip & np.isnan(f), law.f_eq(T_in), f)
        with np.errstate(invalid='ignore'):
            return law.correct(Tst, f, act, skip, cp)

    # -- the device side -------------------------------------------------------------------------------------------------------
    def apply(self, T_star, T_in=None, active=None, skip_k0=False, skip_kN=False):
        """adi_cyl_phase_apply on T_star (a DeviceField or device tensor in the grid's layout), T_star and f in place.  T_in: the
        step's input, from which newborn cells are seeded -- required whenever `active` is given.  skip_k0 / skip_kN: leave the
        plane k = 0 / k = nz - 1 alone (the z sweep pins it when that closure is 'dirichlet')"""
        g = self.grid
        strict = "CylPhaseField.apply: %s must be a fp64 device field in the grid's layout"
        t = _native_f64(g, T_star, strict % "T_star (it is corrected in place)")
        t_in = None if T_in is None else _native_f64(g, T_in, strict % "T_in")
        d_act = _active_arg(g, active)
        if d_act is not None and t_in is None:
            raise ValueError("CylPhaseField.apply: T_in is required with `active` (newborn cells are seeded from it)")
        check(lib.adi_cyl_phase_apply(ctypes.byref(self.law.as_c()), float(self.mat.cp), _p(t), _p(self.f), _p(t_in), _p(d_act),
                                      int(bool(skip_k0)), int(bool(skip_kN)), *g.layout.pd, _stream()))
        return T_star

    def seed(self, T, sel=None, active=None):
        """adi_cyl_phase_seed: f = f_eq(T) on the cells of `active` (None: all) that `sel` selects (None: all of them), NaN off
        `active`; active cells not selected keep f"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        t, d_act = _native_f64(g, T), _active_arg(g, active)          # (held until the launch is queued: they may be copies)
        self._edits += 1
        check(lib.adi_cyl_phase_seed(ctypes.byref(self.law.as_c()), _p(t), _p(self.f), _p(d_act), _p(d_sel), *g.layout.pd,
                                     _stream()))

    @property
    def liquid_fraction(self):
        """a copy of f as a DeviceField of the grid's shape, 0 where the cell has never been active"""
        out = DeviceField(self.f).copy()
        out.t.nan_to_num_(nan=0.0)
        return out

    def snapshot(self):
        return self._flat.clone()

    def restore(self, s):
        self._flat.copy_(s)
        self._edits += 1

    def graph_key(self):
        """what a captured graph holds of the field: the law and cp by value, the buffer by pointer"""
        return (self.law.key(), float(self.mat.cp), self.f.data_ptr())


class CylThermalHistory(_StepRecorder):
    """Thermal history of a GridCyl under HistoryLevels, on the device: `T_peak`, `t_hi`, `t_lo` (fp64, the grid's layout, NaN
    where the cell has never been active and where "never happened"), the melt-pool log (one row of ADI_CYL_HISTORY_LOG_INTS
    integers per recorded step, `capacity` rows and a spill row), the device block (ThermalHistory's: clock and log slot) and
    the host clock `.t`.  T (optional): the field the cells of `active` (None: all) are seeded from; without it every cell is a
    newborn, seeded from the input of the first step that sees it active.
        record(T_in, T_out, dt, active=None)   one step T_in (at .t) -> T_out (at .t + dt): adi_cyl_history_record + the tick
        reset(T, t=0.0, active=None)      seeded from T, the log empty, .t = t
        seed(T, sel=None, active=None)    after an outside edit of already active cells (a birth needs no call)
        snapshot() / restore(s), graph_key(), T_peak, t_hi, t_lo, cooling_time, slot, melt_pool()
    `record_reference` is the definition, adi_cyl_history_record the same operations on the device and
    adi_cyl_history_record_host on the CPU."""

    LOG_GUARD = ThermalHistory.LOG_GUARD
    GUARD_WORD = ThermalHistory.GUARD_WORD
    _keyword = 'history'

    def __init__(self, grid, levels, capacity=4096, T=None, t=0.0, active=None):
        if not isinstance(levels, HistoryLevels):
            raise TypeError("CylThermalHistory: levels must be a HistoryLevels")
        levels.validate()
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("CylThermalHistory: capacity must be >= 1")
        self.grid, self.levels, self.capacity = grid, levels, capacity
        L = grid.layout
        nan = float('nan')
        self._flat = [torch.full((L.numel_padded,), nan, dtype=torch.float64, device=_device()) for _ in range(3)]
        self.d_peak, self.d_t_hi, self.d_t_lo = (f.as_strided(L.shape, L.strides) for f in self._flat)
        n = _lib.CYL_HISTORY_LOG_INTS
        self._log_store = torch.full(((capacity + 1) * n + 2 * self.LOG_GUARD,), self.GUARD_WORD, dtype=torch.int32,
                                     device=_device())
        self.d_log = self._log_store[self.LOG_GUARD:self.LOG_GUARD + (capacity + 1) * n]
        self.d_block = torch.zeros(_lib.HISTORY_BLOCK_BYTES // 8, dtype=torch.int64, device=_device())
        self.t = float(t)
        self._times = []
        self._d_act = None           # the active mask of the step being recorded (the step sets it around _record_step)
        check(lib.adi_cyl_history_reset_log(_p(self.d_block), _p(self.d_log), capacity, _stream()))
        if T is not None:
            self.seed(T, active=active)

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def record_reference(state, A, B, active, t_n, dt, levels):
        """((T_peak, t_hi, t_lo), pool) after the step A -> B from `state`: THE DEFINITION.  active: bool array (None: every
        cell).  The active cells whose T_peak is NaN are newborns and are seeded from A (ThermalHistory.seed_reference with
        sel = active & isnan(T_peak) and an all-true mask); then ThermalHistory.record_reference runs with mask=active.  pool
        carries sum_i, the sum of the radial index i over the pool cells, besides cells, lo and hi."""
        A = np.asarray(A, dtype=np.float64)
        B = np.asarray(B, dtype=np.float64)
        act = np.ones(A.shape, dtype=bool) if active is None else np.asarray(active, dtype=bool)
        peak = np.asarray(state[0], dtype=np.float64)
        seeded = ThermalHistory.seed_reference(state, A, np.ones(A.shape, dtype=bool), sel=act & np.isnan(peak))
        new, pool = ThermalHistory.record_reference(seeded, A, B, act, t_n, dt, levels)
        T_melt = levels.validate()[2]
        pool['sum_i'] = int(np.argwhere(act & (B >= T_melt))[:, 0].sum())
        return new, pool

    @staticmethod
    def pool_row(pool):
        """the log row of a `pool` of record_reference: ADI_CYL_HISTORY_LOG_INTS int32"""
        row = np.zeros(_lib.CYL_HISTORY_LOG_INTS, dtype=np.int32)
        row[0] = pool['cells']
        row[1:4], row[4:7] = pool['lo'], pool['hi']
        row[8:10] = np.array([pool['sum_i']], dtype=np.int64).view(np.int32)
        return row

    @staticmethod
    def pool_volume(grid, cells, sum_i):
        """the volume [m^3] of `cells` pool cells whose radial indices sum to `sum_i`: the sum of r_i dr dphi dz with
        r_i = R_in + (i + 1/2) dr"""
        g = grid
        return g.dphi * g.dz * g.dr * ((g.R_in + 0.5 * g.dr) * np.asarray(cells, dtype=np.float64)
                                       + g.dr * np.asarray(sum_i, dtype=np.float64))

    # -- the device side -------------------------------------------------------------------------------------------------------
    def _check_mask(self):
        pass                                           # (a GridCyl has no mask to synchronise with)

    def _launch_record(self, t_in, t_out):
        g = self.grid
        check(lib.adi_cyl_history_record(ctypes.byref(self.levels.as_c()), _p(self.d_block), _p(t_in), _p(t_out), _p(self.d_peak),
                                         _p(self.d_t_hi), _p(self.d_t_lo), _p(self.d_log), _p(self._d_act), *g.layout.pd,
                                         _stream()))
        check(lib.adi_history_tick(_p(self.d_block), _stream()))

    def record(self, T_in, T_out, dt, active=None):
        """one step T_in (at .t) -> T_out (at .t + dt), both fp64 device fields in the grid's layout, on the cells of `active`
        (None: all): adi_cyl_history_record and the tick; afterwards .t = t0 + dt"""
        self._d_act = _active_arg(self.grid, active)
        try:
            _StepRecorder.record(self, T_in, T_out, dt)
        finally:
            self._d_act = None

    def _record_step(self, t_in, out, dt, captured, d_act=None):
        """what the step calls for "record this step" t_in -> out on the cells of d_act (a uint8 device tensor in the grid's
        layout; None: all).  captured: the record and the tick alone, the caller keeps the clocks; otherwise `record`"""
        if not captured:
            return self.record(t_in, out, dt, active=d_act)
        self._d_act = d_act
        try:
            self._launch_record(t_in, out)
        finally:
            self._d_act = None

    def seed(self, T, sel=None, active=None):
        """adi_cyl_history_seed: T_peak = T, no crossing, on the cells of `active` (None: all) that `sel` selects (None: all of
        them); NaN off `active`"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        t, d_act = _native_f64(g, T), _active_arg(g, active)          # (held until the launch is queued: they may be copies)
        check(lib.adi_cyl_history_seed(_p(t), _p(self.d_peak), _p(self.d_t_hi), _p(self.d_t_lo), _p(d_act), _p(d_sel),
                                       *g.layout.pd, _stream()))

    def reset(self, T, t=0.0, active=None):
        """every cell of `active` seeded from T, the log empty (slot 0), .t = t"""
        self.seed(T, active=active)
        check(lib.adi_cyl_history_reset_log(_p(self.d_block), _p(self.d_log), self.capacity, _stream()))
        self._times = []
        self.t = float(t)

    snapshot = ThermalHistory.snapshot
    restore = ThermalHistory.restore
    graph_key = ThermalHistory.graph_key
    T_peak = ThermalHistory.T_peak
    t_hi = ThermalHistory.t_hi
    t_lo = ThermalHistory.t_lo
    cooling_time = ThermalHistory.cooling_time
    slot = ThermalHistory.slot

    def melt_pool(self):
        """the log over the recorded steps as NumPy arrays: t (end time of each step), cells, lo, hi (int32, (n, 3), as (i, j, k)),
        sum_i (int64: the sum of the radial index over the pool cells), volume = dphi dz dr ((R_in + dr/2) cells + dr sum_i)
        in m^3 -- exact for cells of volume r_i dr dphi dz --, extent_r = (hi_i - lo_i + 1) dr and extent_z = (hi_k - lo_k + 1) dz
        in metres (0 where the pool is empty), and dropped: the steps recorded past the capacity, which the log does not hold.
        lo and hi are plain minima and maxima of the indices: a pool that straddles the seam j = nphi - 1 -> 0 shows lo_j = 0
        and hi_j = nphi - 1, so no extent along phi is reported."""
        return _decode_log(self)
