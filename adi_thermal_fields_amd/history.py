"""Thermal history: the levels `HistoryLevels`, the recorder of peak temperature, cooling time and melt pool, `ThermalHistory`,
and the recorder of the conditions at the freezing front, `SolidificationRecord`; `_StepRecorder`, the clock and the step's
"record this step" call that these two and monitor.py's FieldMonitor share."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _SeededForMask, _device, _native_f64, _p, _stream


# ---- thermal history: peak temperature, cooling time, melt pool (include/adi_hip.h) -------------------
class HistoryLevels:
    """The levels of a thermal-history recorder, in the field's unit: the cooling time is taken between the downward crossings
    of `T_hi` and `T_lo` (T_hi > T_lo; 800 and 500 degrees C give the t8/5 of welding), and a cell with T >= `T_melt` belongs to
    the melt pool.  T_melt is independent of the other two; with a PhaseField one normally passes its liquidus."""

    def __init__(self, T_hi, T_lo, T_melt):
        self.T_hi, self.T_lo, self.T_melt = T_hi, T_lo, T_melt
        self.validate()

    def validate(self):
        """ValueError for anything adi_history_levels rejects (include/adi_hip.h).  -> (T_hi, T_lo, T_melt) as floats"""
        try:
            hi, lo, tm = float(self.T_hi), float(self.T_lo), float(self.T_melt)
        except (TypeError, ValueError):
            raise ValueError("HistoryLevels: T_hi, T_lo and T_melt must be real numbers")
        if not (np.isfinite(hi) and np.isfinite(lo) and np.isfinite(tm)):
            raise ValueError("HistoryLevels: non-finite level")
        if not hi > lo:
            raise ValueError("HistoryLevels: T_hi must be above T_lo")
        return hi, lo, tm

    def as_c(self):
        return _lib.HistoryLevelsC(*self.validate())

    def key(self):
        """every level: a launch takes them by value, so a captured graph holds the levels of its capture"""
        return self.validate()


_POOL_EMPTY_LO = np.iinfo(np.int32).max


# ---- what the step asks of a recorder: ThermalHistory, SolidificationRecord, monitor.py's FieldMonitor ---
class _StepRecorder:
    """The part of a recorder the step drives, written once: a device block of the history's layout (`d_block`), the host clock
    `.t`, the end times `_times` of the recorded steps (None: the recorder keeps none) and `_keyword`, the keyword of the step
    it is passed by, which is how step.py tells a FieldMonitor (a later module) from the other two.  The owner supplies
    `_launch_record(t_in, t_out)` (its record and the tick), `_check_mask`, `snapshot`, `restore`, `graph_key` and `grid`."""
    _keyword = None
    _times = None

    def set_clock(self, dt):
        """the block's clock from the host clock: t0 = .t, this dt, n = 0 (the log slot, if there is one, stays)"""
        check(lib.adi_history_set_clock(_p(self.d_block), self.t, float(dt), _stream()))

    def advance_clock(self, t0, dt, nsteps):
        """host side of `nsteps` recorded steps of dt from t0: their end times join the log's, .t = t0 + nsteps*dt"""
        if self._times is not None:
            self._times.extend(t0 + (n + 1) * dt for n in range(nsteps))
        self.t = t0 + nsteps * dt

    def record(self, T_in, T_out, dt):
        """one step T_in (at .t) -> T_out (at .t + dt), both fp64 device fields in the grid's layout: one record launch and the
        tick; afterwards .t = t0 + dt"""
        strict = "%s.record: T_in and T_out must be fp64 device fields in the grid's layout" % type(self).__name__
        t_in, t_out = _native_f64(self.grid, T_in, strict), _native_f64(self.grid, T_out, strict)
        self._check_mask()
        dt = float(dt)
        self.set_clock(dt)
        self._launch_record(t_in, t_out)
        self.advance_clock(self.t, dt, 1)

    def _record_step(self, t_in, out, dt, captured):
        """what the step calls for "record this step" t_in -> out.  captured: a graph may replay the launches and the caller
        keeps the clocks, so the record and the tick alone; otherwise the public `record`"""
        if captured:
            self._launch_record(t_in, out)
        else:
            self.record(t_in, out, dt)


class ThermalHistory(_SeededForMask, _StepRecorder):
    """Thermal history of a grid under HistoryLevels, on the device: `T_peak`, `t_hi`, `t_lo` (fp64, the grid's layout, NaN off
    the mask and where "never happened"), the melt-pool log (one row of ADI_HISTORY_LOG_INTS integers per recorded step, `capacity`
    rows and a spill row), the device block (clock and log slot) and the host clock `.t`: the time at which the next recorded
    step starts.  Every buffer lives as long as the object, so a StagedStepper's graph holds their pointers.  T (optional): the
    field the state is seeded from; without it nothing is seeded and `reset(T)` must come before the first record.
        record(T_in, T_out, dt)   one step T_in (at .t) -> T_out (at .t + dt): adi_history_record + adi_history_tick
        reset(T, t=0.0)           T_peak = T on the mask, no crossing anywhere, the log empty, .t = t
        sync_mask(T)              after `grid.mask` changed or T was edited on newborn cells: those that joined the mask are
                                  seeded from T, those that left it become NaN, every other cell keeps its state
        snapshot() / restore(s)   the fields, the log, the block and the host clock
        T_peak, t_hi, t_lo, cooling_time     copies as DeviceField;  melt_pool()   the log as NumPy arrays
    `record_reference` is the definition, adi_history_record the same operations on the device."""

    LOG_GUARD = 8        # integers either side of the log that no launch may touch (tests read them)
    GUARD_WORD = 0x5a5a5a5a
    _keyword = 'history'

    def __init__(self, grid, levels, capacity=4096, T=None, t=0.0):
        if not isinstance(levels, HistoryLevels):
            raise TypeError("ThermalHistory: levels must be a HistoryLevels")
        levels.validate()
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("ThermalHistory: capacity must be >= 1")
        self.grid, self.levels, self.capacity = grid, levels, capacity
        L = grid.layout
        nan = float('nan')
        self._flat = [torch.full((L.numel_padded,), nan, dtype=torch.float64, device=_device()) for _ in range(3)]
        self.d_peak, self.d_t_hi, self.d_t_lo = (f.as_strided(L.shape, L.strides) for f in self._flat)
        n = _lib.HISTORY_LOG_INTS
        self._log_store = torch.full(((capacity + 1) * n + 2 * self.LOG_GUARD,), self.GUARD_WORD, dtype=torch.int32,
                                     device=_device())
        self.d_log = self._log_store[self.LOG_GUARD:self.LOG_GUARD + (capacity + 1) * n]
        self.d_block = torch.zeros(_lib.HISTORY_BLOCK_BYTES // 8, dtype=torch.int64, device=_device())
        self.t = float(t)
        self._times = []             # end time of every recorded step, host side
        check(lib.adi_history_reset_log(_p(self.d_block), _p(self.d_log), capacity, _stream()))
        if T is not None:
            self.reset(T, t)

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def record_reference(state, A, B, mask, t_n, dt, levels):
        """((T_peak, t_hi, t_lo), pool) after the step A (the field at t_n) -> B (the step's final result, after the latent-heat
        correction if there is one, at t_n + dt) from `state` = (T_peak, t_hi, t_lo): THE DEFINITION of the recorder -- one fp64
        operation per line, in the order the kernel performs them.  In-mask cells only; off-mask cells keep their state bit for
        bit.  "Never happened" and "off the mask" are NaN in all three fields.  pool = dict(cells, lo, hi): the number of
        in-mask cells with B >= T_melt and the smallest / largest (i, j, k) among them (cells = 0, lo = INT32_MAX, hi = -1 when
        there is none).  t_n is formed by the caller as t0 + n*dt, n the step index within the current run.
        Precondition (the kernel's skip rule -- a brick none of whose peaks exceeds T_lo is not looked at for crossings -- is
        exact under it): every in-mask value of A has been recorded, A <= T_peak.  It holds when the recorder follows every
        step and reset / sync_mask follows every outside edit of T."""
        T_hi, T_lo, T_melt = levels.validate()
        peak, t_hi, t_lo = (np.asarray(s, dtype=np.float64) for s in state)
        A = np.asarray(A, dtype=np.float64)
        B = np.asarray(B, dtype=np.float64)
        m = np.asarray(mask, dtype=bool)
        t_n, dt = float(t_n), float(dt)
        # 1. the peak
        peak_n = np.where(m & (B > peak), B, peak)
        with np.errstate(divide='ignore', invalid='ignore'):
            den = A - B
            # 2. downward crossing of T_hi: a new cooling cycle
            c_hi = m & (A > T_hi) & (B <= T_hi)
            num = A - T_hi
            fr = num / den
            off = dt * fr
            tc = t_n + off
            t_hi_n = np.where(c_hi, tc, t_hi)
            t_lo_n = np.where(c_hi, np.nan, t_lo)
            # 3. downward crossing of T_lo
            c_lo = m & (A > T_lo) & (B <= T_lo)
            num = A - T_lo
            fr = num / den
            off = dt * fr
            tc = t_n + off
            t_lo_n = np.where(c_lo, tc, t_lo_n)
        # 4. the melt pool of the step
        idx = np.argwhere(m & (B >= T_melt))
        if len(idx):
            pool = dict(cells=int(len(idx)), lo=idx.min(axis=0).astype(np.int32), hi=idx.max(axis=0).astype(np.int32))
        else:
            pool = dict(cells=0, lo=np.full(3, _POOL_EMPTY_LO, dtype=np.int32), hi=np.full(3, -1, dtype=np.int32))
        return (peak_n, t_hi_n, t_lo_n), pool

    @staticmethod
    def seed_reference(state, T, mask, sel=None):
        """the state after adi_history_seed: T_peak = T and NaN times on the in-mask cells `sel` selects (None: all), NaN off
        the mask, every other cell unchanged"""
        m = np.asarray(mask, dtype=bool)
        s = m if sel is None else (m & np.asarray(sel, dtype=bool))
        peak, t_hi, t_lo = (np.where(m, np.asarray(a, dtype=np.float64), np.nan) for a in state)
        return np.where(s, np.asarray(T, dtype=np.float64), peak), np.where(s, np.nan, t_hi), np.where(s, np.nan, t_lo)

    # -- the device side -------------------------------------------------------------------------------------------------------
    def _launch_record(self, t_in, t_out):
        g = self.grid
        check(lib.adi_history_record(ctypes.byref(self.levels.as_c()), _p(self.d_block), _p(t_in), _p(t_out), _p(self.d_peak),
                                     _p(self.d_t_hi), _p(self.d_t_lo), _p(self.d_log), _p(g.d_flags), _p(g.d_bricks),
                                     *g.layout.pd, _stream()))
        check(lib.adi_history_tick(_p(self.d_block), _stream()))

    def _check_mask(self):
        if self.grid.mask_version != self._mask_version:
            raise ValueError("ThermalHistory: the grid's mask changed since the history was seeded; call sync_mask(T)")

    def seed(self, T, sel=None):
        """adi_history_seed: T_peak = T, no crossing, on the in-mask cells `sel` selects (None: every in-mask cell); NaN off the
        mask"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        check(lib.adi_history_seed(_p(_native_f64(g, T)), _p(self.d_peak), _p(self.d_t_hi), _p(self.d_t_lo),
                                   _p(g.d_flags), _p(g.d_bricks), _p(d_sel), *g.layout.pd, _stream()))
        self._remember_mask()

    def reset(self, T, t=0.0):
        """every in-mask cell seeded from T, the log empty (slot 0), .t = t"""
        self.seed(T)
        check(lib.adi_history_reset_log(_p(self.d_block), _p(self.d_log), self.capacity, _stream()))
        self._times = []
        self.t = float(t)

    def snapshot(self):
        return [f.clone() for f in self._flat], self._log_store.clone(), self.d_block.clone(), self.t, list(self._times)

    def restore(self, s):
        for f, held in zip(self._flat, s[0]):
            f.copy_(held)
        self._log_store.copy_(s[1])
        self.d_block.copy_(s[2])
        self.t = s[3]
        self._times = list(s[4])

    def graph_key(self):
        """what a captured graph holds of the recorder: the levels by value, the buffers by pointer"""
        return (self.levels.key(), self.d_peak.data_ptr(), self.d_t_hi.data_ptr(), self.d_t_lo.data_ptr(),
                self.d_log.data_ptr(), self.d_block.data_ptr())

    T_peak = property(lambda self: DeviceField(self.d_peak).copy())
    t_hi = property(lambda self: DeviceField(self.d_t_hi).copy())
    t_lo = property(lambda self: DeviceField(self.d_t_lo).copy())

    @property
    def cooling_time(self):
        """t_lo - t_hi: NaN until a cycle completes"""
        out = self.t_lo
        out.t.sub_(self.d_t_hi)
        return out

    @property
    def slot(self):
        """steps recorded since the last reset (read from the device block)"""
        return int(self.d_block.cpu()[3].item())

    def melt_pool(self):
        """the log over the recorded steps as NumPy arrays: t (end time of each step), cells, lo, hi (int32, (n, 3)), extent =
        (hi - lo + 1)*dx in metres (0 where the pool is empty), volume = cells*dx^3, and dropped: the steps recorded past the
        capacity, which the log does not hold"""
        slot = self.slot
        n = min(slot, self.capacity)
        rows = self.d_log.cpu().numpy().reshape(self.capacity + 1, _lib.HISTORY_LOG_INTS)[:n]
        cells, lo, hi = rows[:, 0].copy(), rows[:, 1:4].copy(), rows[:, 4:7].copy()
        dx = self.grid.dx
        extent = np.where((cells > 0)[:, None], (hi.astype(np.int64) - lo.astype(np.int64) + 1) * dx, 0.0)
        return dict(t=np.asarray(self._times[:n], dtype=np.float64), cells=cells, lo=lo, hi=hi, extent=extent,
                    volume=cells * dx ** 3, dropped=max(0, slot - self.capacity))


# ---- the freezing front: thermal gradient and cooling rate at solidification (include/adi_hip.h) --------
class SolidificationRecord(_SeededForMask, _StepRecorder):
    """The conditions at the solidification front of a grid, on the device: per cell, taken at the moment the cell last froze
    (dropped from above `T_freeze` to it or below within one step), the crossing time `t_solid`, the cooling rate and the
    SQUARE of the thermal gradient, `g2` (fp64, the grid's layout, NaN off the mask and where the cell never froze); the word per
    16^3 brick that lets a cold brick skip the load of the step's input; the device block (clock) and the host clock `.t`: the
    time at which the next recorded step starts.  Every buffer lives as long as the object, so a StagedStepper's graph holds
    their pointers.  T (optional): the field the brick words are seeded from; without it `reset(T)` must come before the first
    record.
        record(T_in, T_out, dt)   one step T_in (at .t) -> T_out (at .t + dt): adi_solid_record + adi_history_tick
        reset(T, t=0.0)           no cell has frozen, the brick words from T, .t = t
        sync_mask(T)              after `grid.mask` changed or T was edited on newborn cells: those that joined the mask are
                                  seeded (NaN; their brick's word set where T > T_freeze), those that left it become NaN
        snapshot() / restore(s)   the fields, the brick words, the block and the host clock
        t_solid, cooling_rate, g2 copies as DeviceField
        G                         sqrt(g2), the thermal gradient |grad T| at the crossing time
        R                         cooling_rate / G, the speed of the front; inf where G = 0 (a cell with no neighbour in the
                                  mask, or a flat field): such a cell cools without a front passing through it
    `record_reference` is the definition, adi_solid_record the same operations on the device.  The device stores G squared so
    that every stored number comes from + - * / alone and is held to bit equality; the square root is taken here.  It keeps no
    list of end times (there is no log to go with them): `_times` stays None."""
    _keyword = 'solidification'

    def __init__(self, grid, T_freeze, T=None, t=0.0):
        self.grid, self.T_freeze = grid, self._level(T_freeze)
        L = grid.layout
        nan = float('nan')
        self._flat = [torch.full((L.numel_padded,), nan, dtype=torch.float64, device=_device()) for _ in range(3)]
        self.d_t_solid, self.d_rate, self.d_g2 = (f.as_strided(L.shape, L.strides) for f in self._flat)
        nb = [(n + _lib.BRICK - 1) // _lib.BRICK for n in L.pd[:3]]
        self.d_hot = torch.zeros(nb[0] * nb[1] * nb[2], dtype=torch.int32, device=_device())
        self.d_block = torch.zeros(_lib.HISTORY_BLOCK_BYTES // 8, dtype=torch.int64, device=_device())
        self.t = float(t)
        if T is not None:
            self.reset(T, t)

    @staticmethod
    def _level(T_freeze):
        try:
            tf = float(T_freeze)
        except (TypeError, ValueError):
            raise ValueError("SolidificationRecord: T_freeze must be a real number")
        if not np.isfinite(tf):
            raise ValueError("SolidificationRecord: non-finite T_freeze")
        return tf

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def record_reference(state, A, B, mask, t_n, dt, dx, T_freeze):
        """(t_solid, cooling_rate, g2) after the step A (the field at t_n) -> B (the step's final result, after any latent-heat or
        material-law recovery, at t_n + dt) from `state` = (t_solid, cooling_rate, g2): THE DEFINITION of the recorder -- one fp64
        operation per line, in the order the kernel performs them.  An in-mask cell freezes in this step exactly when
        A > T_freeze and B <= T_freeze; every other cell keeps its state bit for bit, and a cell that freezes again is
        overwritten.  The gradient of A and of B is central where both neighbours along an axis are in the mask, one-sided where
        one is, 0 where none is (a box face counts as absent), and is interpolated to the crossing time.  t_n is formed by the
        caller as t0 + n*dt, n the step index within the current run.
        Precondition (the kernel's skip rule -- A is loaded only in bricks that held an in-mask B above T_freeze at the previous
        record -- is exact under it): this step's A is the previous record's B on the mask.  It holds when the recorder follows
        every step and reset / sync_mask follows every outside edit of T."""
        T_f = SolidificationRecord._level(T_freeze)
        t_solid, rate, g2 = (np.asarray(s, dtype=np.float64) for s in state)
        A = np.asarray(A, dtype=np.float64)
        B = np.asarray(B, dtype=np.float64)
        m = np.asarray(mask, dtype=bool)
        t_n, dt, dx = float(t_n), float(dt), float(dx)
        two_dx = 2.0 * dx
        fz = m & (A > T_f) & (B <= T_f)
        mp = np.pad(m, 1)

        def shifted(a, axis, d):
            """the padded array `a` read at the neighbour d = -1 / +1 along `axis`, on the shape of the grid"""
            return a[tuple(slice(1 + (d if i == axis else 0), 1 + (d if i == axis else 0) + n) for i, n in enumerate(m.shape))]

        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            den = A - B
            num = A - T_f
            fr = num / den
            off = dt * fr
            tc = t_n + off
            cr = den / dt
            g = []
            for axis in range(3):
                lo, hi = shifted(mp, axis, -1), shifted(mp, axis, +1)
                both, hi_only, lo_only = lo & hi, hi & ~lo, lo & ~hi
                ga_gb = []
                for F in (A, B):
                    Fp = np.pad(F, 1)
                    minus, plus = shifted(Fp, axis, -1), shifted(Fp, axis, +1)
                    d = np.where(both, plus - minus, np.where(hi_only, plus - F, F - minus))
                    ga_gb.append(np.where(both, d / two_dx, np.where(hi_only | lo_only, d / dx, 0.0)))
                gA, gB = ga_gb
                dg = gB - gA
                sg = fr * dg
                g.append(gA + sg)
            xx = g[0] * g[0]
            yy = g[1] * g[1]
            zz = g[2] * g[2]
            s = xx + yy
            g2_n = s + zz
        return np.where(fz, tc, t_solid), np.where(fz, cr, rate), np.where(fz, g2_n, g2)

    @staticmethod
    def seed_reference(state, T, mask, sel=None):
        """the state after adi_solid_seed: all three fields NaN on the in-mask cells `sel` selects (None: all) and off the mask,
        every other cell unchanged (T only feeds the brick words, which are no part of the state)"""
        m = np.asarray(mask, dtype=bool)
        s = m if sel is None else (m & np.asarray(sel, dtype=bool))
        return tuple(np.where(m & ~s, np.asarray(a, dtype=np.float64), np.nan) for a in state)

    # -- the device side -------------------------------------------------------------------------------------------------------
    def _launch_record(self, t_in, t_out):
        g = self.grid
        check(lib.adi_solid_record(self._level(self.T_freeze), g.dx, _p(self.d_block), _p(t_in), _p(t_out), _p(self.d_t_solid),
                                   _p(self.d_rate), _p(self.d_g2), _p(self.d_hot), _p(g.d_flags), _p(g.d_bricks),
                                   *g.layout.pd, _stream()))
        check(lib.adi_history_tick(_p(self.d_block), _stream()))

    def _check_mask(self):
        if self.grid.mask_version != self._mask_version:
            raise ValueError("SolidificationRecord: the grid's mask changed since the record was seeded; call sync_mask(T)")

    def seed(self, T, sel=None):
        """adi_solid_seed: "never froze" on the in-mask cells `sel` selects (None: every in-mask cell), NaN off the mask; the word
        of a brick is set where one of those cells has T > T_freeze, and a word that is set stays set"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        check(lib.adi_solid_seed(self._level(self.T_freeze), _p(_native_f64(g, T)), _p(self.d_t_solid), _p(self.d_rate),
                                 _p(self.d_g2), _p(self.d_hot), _p(g.d_flags), _p(g.d_bricks), _p(d_sel), *g.layout.pd,
                                 _stream()))
        self._remember_mask()

    def reset(self, T, t=0.0):
        """no cell has frozen, the brick words rebuilt from T alone, .t = t"""
        self.d_hot.zero_()
        self.seed(T)
        self.t = float(t)

    def snapshot(self):
        return [f.clone() for f in self._flat], self.d_hot.clone(), self.d_block.clone(), self.t

    def restore(self, s):
        for f, held in zip(self._flat, s[0]):
            f.copy_(held)
        self.d_hot.copy_(s[1])
        self.d_block.copy_(s[2])
        self.t = s[3]

    def graph_key(self):
        """what a captured graph holds of the recorder: T_freeze and dx by value, the buffers by pointer"""
        return (self._level(self.T_freeze), self.grid.dx, self.d_t_solid.data_ptr(), self.d_rate.data_ptr(),
                self.d_g2.data_ptr(), self.d_hot.data_ptr(), self.d_block.data_ptr())

    t_solid = property(lambda self: DeviceField(self.d_t_solid).copy())
    cooling_rate = property(lambda self: DeviceField(self.d_rate).copy())
    g2 = property(lambda self: DeviceField(self.d_g2).copy())

    @property
    def G(self):
        """sqrt(g2): NaN where the cell never froze"""
        out = DeviceField(self.d_g2).copy()
        out.t.sqrt_()
        return out

    @property
    def R(self):
        """cooling_rate / G; inf where G = 0"""
        out = self.cooling_rate
        out.t.div_(torch.sqrt(self.d_g2))
        return out
