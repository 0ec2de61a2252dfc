"""The freezing front of the cylindrical step: `CylSolidificationRecord`, the recorder of crossing time, cooling rate and
|grad T|^2 per cell at the moment the cell last froze, with a per-step log of the front (include/adi_hip.h, "Solidification record
of the cylindrical step").  The law is the Cartesian SolidificationRecord's; the conventions are the
cylindrical backend's: the metric puts r_i dphi under the phi difference, phi is periodic (the seam is no box face), `active`
is an optional per-call array (None: every cell), and NaN means "never froze" whether or not the cell was ever active -- so
there is no seeding, no sync, and a birth needs no call."""
import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _device, _native_f64, _p, _stream
from .history import SolidificationRecord, ThermalHistory, _StepRecorder, _POOL_EMPTY_LO
from .cyl_extras import CylThermalHistory, _active_arg, _decode_log


class CylSolidificationRecord(_StepRecorder):
    """The conditions at the solidification front of a GridCyl, on the device: per cell, taken at the moment the cell last froze
    (dropped from above `T_freeze` to it or below within one step), the crossing time `t_solid`, the cooling rate and the SQUARE
    of the thermal gradient, `g2` (fp64, the grid's layout, NaN where the cell never froze); the front log (one row of
    ADI_CYL_HISTORY_LOG_INTS integers per recorded step over the cells that froze in it, `capacity` rows and a spill row); one
    hot word per tile of ADI_CYL_SOLID_TILE cells of a (phi, z) plane, which lets a cold tile skip the load of the step's input;
    the device block (clock and log slot) and the host clock `.t`.  Every buffer lives as long as the object, so a
    StagedCylStepper's graph holds their pointers.
        record(T_in, T_out, dt, active=None)   one step T_in (at .t) -> T_out (at .t + dt): adi_cyl_solid_record + the tick
        reset(t=0.0)                      no cell has frozen, the log empty, .t = t
        seed_hot(T, active=None)          the hot words from a field (adi_cyl_solid_hot_seed)
        snapshot() / restore(s), graph_key(), slot, t_solid, cooling_rate, g2, G, R, front()
    The hot words are exact only while every record's input is bitwise the previous record's result (or the seeded field) on
    the same active cells, which a birth breaks: `record` and the plain steps pass none, StagedCylStepper.run seeds them from
    its input and passes them (record(..., hot=True) does the same by hand).
    `record_reference` is the definition, adi_cyl_solid_record the same operations on the device and adi_cyl_solid_record_host
    on the CPU.  The device stores G squared so that every stored number comes from + - * / alone and is held to bit equality;
    the square root is taken here."""

    LOG_GUARD = ThermalHistory.LOG_GUARD
    GUARD_WORD = ThermalHistory.GUARD_WORD
    _keyword = 'solidification'
    use_hot_words = True             # False: StagedCylStepper.run passes no hot words either (what the cost probe compares with)

    def __init__(self, grid, T_freeze, capacity=4096, t=0.0):
        self.grid, self.T_freeze = grid, SolidificationRecord._level(T_freeze)
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("CylSolidificationRecord: capacity must be >= 1")
        self.capacity = capacity
        L = grid.layout
        nan = float('nan')
        self._flat = [torch.full((L.numel_padded,), nan, dtype=torch.float64, device=_device()) for _ in range(3)]
        self.d_t_solid, self.d_rate, self.d_g2 = (f.as_strided(L.shape, L.strides) for f in self._flat)
        n = _lib.CYL_HISTORY_LOG_INTS
        self._log_store = torch.full(((capacity + 1) * n + 2 * self.LOG_GUARD,), self.GUARD_WORD, dtype=torch.int32,
                                     device=_device())
        self.d_log = self._log_store[self.LOG_GUARD:self.LOG_GUARD + (capacity + 1) * n]
        words = self.hot_words(grid.shape)
        self._hot_store = torch.full((words + 2 * self.LOG_GUARD,), self.GUARD_WORD, dtype=torch.int32, device=_device())
        self.d_hot = self._hot_store[self.LOG_GUARD:self.LOG_GUARD + words]
        self.d_hot.fill_(1)          # (a set word only costs the full path: exact whatever the field)
        self.d_block = torch.zeros(_lib.HISTORY_BLOCK_BYTES // 8, dtype=torch.int64, device=_device())
        self.t = float(t)
        self._times = []
        self._d_act = None           # the active mask of the step being recorded (the step sets it around _record_step)
        self._hot = False            # whether the launch being issued passes the hot words
        check(lib.adi_cyl_history_reset_log(_p(self.d_block), _p(self.d_log), capacity, _stream()))

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def hot_words(shape):
        """the number of hot words of a grid of this shape: nr * ceil(nphi*nz / ADI_CYL_SOLID_TILE)"""
        nr, nphi, nz = shape
        return nr * ((nphi * nz + _lib.CYL_SOLID_TILE - 1) // _lib.CYL_SOLID_TILE)

    @staticmethod
    def record_reference(state, A, B, active, t_n, dt, grid, T_freeze):
        """((t_solid, cooling_rate, g2), front) after the step A (the field at t_n) -> B (the step's final result, at t_n + dt)
        from `state` = (t_solid, cooling_rate, g2): THE DEFINITION of the recorder -- SolidificationRecord.record_reference in
        the cylindrical metric, one fp64 operation per line, in the order the kernel performs them.  active: bool array (None:
        every cell).  A cell of `active` freezes in this step exactly when A > T_freeze and B <= T_freeze; every other cell
        keeps its state bit for bit, and a cell that freezes again is overwritten.  The steps are dr, r_i dphi with
        r_i = R_in + ((i + 0.5) dr), and dz.  The neighbours are i -+ 1 and k -+ 1 inside the box (a box face counts as absent)
        and (j -+ 1) mod nphi -- none with nphi == 1; with nphi == 2 both are the same cell and the central difference is
        +0.0.  A neighbour is present only where `active` holds it.  The gradient of A and of B is central where both
        neighbours are present, one-sided where one is, 0 where none is, and is interpolated to the crossing time.
        front = dict(cells, lo, hi, sum_i) over the cells that froze in this step: their number, the smallest / largest
        (i, j, k) and the sum of the radial index (cells = 0, lo = INT32_MAX, hi = -1, sum_i = 0 when none did)."""
        T_f = SolidificationRecord._level(T_freeze)
        t_solid, rate, g2 = (np.asarray(s, dtype=np.float64) for s in state)
        A = np.asarray(A, dtype=np.float64)
        B = np.asarray(B, dtype=np.float64)
        m = np.ones(A.shape, dtype=bool) if active is None else np.asarray(active, dtype=bool)
        t_n, dt = float(t_n), float(dt)
        nr, nphi, nz = A.shape
        ih = np.arange(nr, dtype=np.float64) + 0.5
        ro = ih * float(grid.dr)
        r = float(getattr(grid, 'R_in', 0.0)) + ro
        h_phi = (r * float(grid.dphi))[:, None, None]
        hs = (float(grid.dr), h_phi, float(grid.dz))
        fz = m & (A > T_f) & (B <= T_f)

        def nbr(a, axis, d, fill):
            """`a` read at the neighbour d = -1 / +1 along `axis`: periodic along phi, `fill` past a box face"""
            if axis == 1:
                return np.roll(a, -d, axis=1)
            out = np.full(a.shape, fill, dtype=a.dtype)
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis] = slice(1, None) if d > 0 else slice(None, -1)
            dst[axis] = slice(None, -1) if d > 0 else slice(1, None)
            out[tuple(dst)] = a[tuple(src)]
            return out

        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            den = A - B
            num = A - T_f
            fr = num / den
            off = dt * fr
            tc = t_n + off
            cr = den / dt
            g = []
            for axis in range(3):
                h = hs[axis]
                two_h = 2.0 * h
                if axis == 1 and nphi == 1:
                    lo = hi = np.zeros(A.shape, dtype=bool)          # (a cell is not its own neighbour)
                else:
                    lo, hi = nbr(m, axis, -1, False), nbr(m, axis, +1, False)
                both, hi_only, lo_only = lo & hi, hi & ~lo, lo & ~hi
                ga_gb = []
                for F in (A, B):
                    minus, plus = nbr(F, axis, -1, 0.0), nbr(F, axis, +1, 0.0)
                    d = np.where(both, plus - minus, np.where(hi_only, plus - F, F - minus))
                    ga_gb.append(np.where(both, d / two_h, np.where(hi_only | lo_only, d / h, 0.0)))
                gA, gB = ga_gb
                dg = gB - gA
                sg = fr * dg
                g.append(gA + sg)
            rr = g[0] * g[0]
            pp = g[1] * g[1]
            zz = g[2] * g[2]
            s = rr + pp
            g2_n = s + zz
        idx = np.argwhere(fz)
        if len(idx):
            front = dict(cells=int(len(idx)), lo=idx.min(axis=0).astype(np.int32), hi=idx.max(axis=0).astype(np.int32),
                         sum_i=int(idx[:, 0].sum()))
        else:
            front = dict(cells=0, lo=np.full(3, _POOL_EMPTY_LO, dtype=np.int32), hi=np.full(3, -1, dtype=np.int32), sum_i=0)
        return (np.where(fz, tc, t_solid), np.where(fz, cr, rate), np.where(fz, g2_n, g2)), front

    front_row = staticmethod(CylThermalHistory.pool_row)      # the log row of a `front` of record_reference

    @staticmethod
    def hot_reference(T, active, T_freeze, shape):
        """the hot words after a record whose result was T, or after seed_hot(T): int32, one per tile, 1 where some cell of
        `active` (None: every cell) in the tile has T > T_freeze"""
        nr, nphi, nz = shape
        T = np.asarray(T, dtype=np.float64).reshape(nr, nphi * nz)
        m = np.ones(T.shape, dtype=bool) if active is None else np.asarray(active, dtype=bool).reshape(nr, nphi * nz)
        above = m & (T > float(T_freeze))
        tile = _lib.CYL_SOLID_TILE
        ntile = (nphi * nz + tile - 1) // tile
        padded = np.zeros((nr, ntile * tile), dtype=bool)
        padded[:, :nphi * nz] = above
        return padded.reshape(nr, ntile, tile).any(axis=2).astype(np.int32).reshape(-1)

    # -- the device side -------------------------------------------------------------------------------------------------------
    def _check_mask(self):
        pass                                           # (a GridCyl has no mask to synchronise with)

    def _launch_record(self, t_in, t_out):
        g = self.grid
        check(lib.adi_cyl_solid_record(self.T_freeze, g.R_in, g.dr, g.dphi, g.dz, _p(self.d_block), _p(t_in), _p(t_out),
                                       _p(self.d_t_solid), _p(self.d_rate), _p(self.d_g2), _p(self.d_log), _p(self._d_act),
                                       _p(self.d_hot if self._hot else None), *g.layout.pd, _stream()))
        check(lib.adi_history_tick(_p(self.d_block), _stream()))

    def record(self, T_in, T_out, dt, active=None, hot=False):
        """one step T_in (at .t) -> T_out (at .t + dt), both fp64 device fields in the grid's layout, on the cells of `active`
        (None: all): adi_cyl_solid_record and the tick; afterwards .t = t0 + dt.  hot: pass the hot words -- only where T_in is
        bitwise the field of the last record(hot=True) or seed_hot on the same `active`"""
        self._d_act, self._hot = _active_arg(self.grid, active), bool(hot) and self.use_hot_words
        try:
            _StepRecorder.record(self, T_in, T_out, dt)
        finally:
            self._d_act, self._hot = None, False

    def _record_step(self, t_in, out, dt, captured, d_act=None, hot=False):
        """what the step calls for "record this step" t_in -> out on the cells of d_act (a uint8 device tensor in the grid's
        layout; None: all).  captured: the record and the tick alone, the caller keeps the clocks; otherwise `record`"""
        if not captured:
            return self.record(t_in, out, dt, active=d_act, hot=hot)
        self._d_act, self._hot = d_act, bool(hot) and self.use_hot_words
        try:
            self._launch_record(t_in, out)
        finally:
            self._d_act, self._hot = None, False

    def seed_hot(self, T, active=None):
        """adi_cyl_solid_hot_seed: every hot word from T on the cells of `active` (None: all)"""
        g = self.grid
        t, d_act = _native_f64(g, T), _active_arg(g, active)          # (held until the launch is queued: they may be copies)
        check(lib.adi_cyl_solid_hot_seed(self.T_freeze, _p(t), _p(d_act), _p(self.d_hot), *g.layout.pd, _stream()))

    def reset(self, t=0.0):
        """no cell has frozen, the log empty (slot 0), every hot word set, .t = t"""
        for f in self._flat:
            f.fill_(float('nan'))
        self.d_hot.fill_(1)
        check(lib.adi_cyl_history_reset_log(_p(self.d_block), _p(self.d_log), self.capacity, _stream()))
        self._times = []
        self.t = float(t)

    def snapshot(self):
        return ([f.clone() for f in self._flat], self._log_store.clone(), self.d_block.clone(), self.t, list(self._times),
                self._hot_store.clone())

    def restore(self, s):
        ThermalHistory.restore(self, s)
        self._hot_store.copy_(s[5])

    def graph_key(self):
        """what a captured graph holds of the recorder: T_freeze and the four geometry numbers by value, the buffers by pointer,
        and whether the hot words are passed"""
        g = self.grid
        return (self.T_freeze, g.R_in, g.dr, g.dphi, g.dz, self.d_t_solid.data_ptr(), self.d_rate.data_ptr(),
                self.d_g2.data_ptr(), self.d_log.data_ptr(), self.d_hot.data_ptr(), self.d_block.data_ptr(),
                bool(self.use_hot_words))

    slot = ThermalHistory.slot
    t_solid = property(lambda self: DeviceField(self.d_t_solid).copy())
    cooling_rate = property(lambda self: DeviceField(self.d_rate).copy())
    g2 = property(lambda self: DeviceField(self.d_g2).copy())
    G = SolidificationRecord.G
    R = SolidificationRecord.R

    def front(self):
        """the log over the recorded steps as NumPy arrays, what CylThermalHistory.melt_pool returns, for the cells that froze
        in each step: t (end time of the step), cells, lo, hi (int32, (n, 3), as (i, j, k)), sum_i, the exact volume [m^3]
        (CylThermalHistory.pool_volume), extent_r, extent_z [m] and dropped"""
        return _decode_log(self)
