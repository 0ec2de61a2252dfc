"""The field monitor of the cylindrical step, `CylFieldMonitor`: probe temperatures, the extrema and the r-weighted sums of
index boxes whose phi range may wrap the seam, one row of a device log per recorded step (include/adi_hip.h, "Field monitor of
the cylindrical step").  The conventions are the cylindrical backend's, as in cyl_extras.py: `active` is an
optional per-call array (None: every cell), there is no per-cell state and no mask version, and a birth needs no call."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import _device, _native_f64, _p, _stream
from .history import _StepRecorder
from .monitor import FieldMonitor
from .cyl_extras import CylThermalHistory, _active_arg


class CylFieldMonitor(_StepRecorder):
    """What a cylindrical run is calibrated and checked with, logged on the device after every recorded step: the step's final
    field at up to 256 `probes` (cells (i, j, k); NaN while the cell is not active) and, over the active cells of 1 to 8
    `regions` (half-open index boxes ((i0, i1), (j0, j1), (k0, k1)); None, also what an empty `regions` means: the whole grid;
    the phi range may wrap the seam: 0 <= j0 < nphi, j0 < j1 <= j0 + nphi, the cells j mod nphi; they may overlap): `cells`,
    `sum_i` (the sum of the radial index), `T_min`, `T_max` (NaN when cells == 0), `sum_T`, `sum_rT` (r_i = R_in + (i + 1/2) dr)
    and, with `extra` (an fp64 device field in the grid's layout, held by pointer: CylPhaseField.f, say, whose NaN "never
    seeded" counts as 0), `sum_extra` and `sum_rextra`.  The log has `capacity` rows and a spill row; the block and the host
    clock `.t` are the thermal history's.
        record(T_out, dt, active=None)   one row from T_out at the block's slot, then the tick; record(T0, 0.0) logs the initial state
        reset(t=0.0)              the log empty (slot 0), .t = t
        snapshot() / restore(s)   the log, the block and the host clock
        traces()                  t and T[probe, step]
        region_log(mat=None)      t, cells, T_min, T_max, sum_T, T_mean, volume, T_vmean, heat, extra_volume ([region, step]), dropped
    `record_reference` is the definition, adi_cyl_monitor_record the same operations on the device and
    adi_cyl_monitor_record_host on the CPU.
    Not covered: probes between cell centres; where the extremum lies; regions given by a label field; control loops that read
    the log."""

    LOG_GUARD = FieldMonitor.LOG_GUARD
    GUARD_WORD = FieldMonitor.GUARD_WORD
    MAX_PROBES = _lib.MONITOR_MAX_PROBES
    MAX_REGIONS = _lib.MONITOR_MAX_REGIONS
    REGION_WORDS = _lib.CYL_MONITOR_REGION_WORDS
    NAMES = ('cells', 'sum_i', 'T_min', 'T_max', 'sum_T', 'sum_rT', 'sum_extra', 'sum_rextra')
    _keyword = 'monitor'

    def __init__(self, grid, probes=(), regions=(), capacity=4096, extra=None, t=0.0):
        shape = tuple(grid.shape)
        self.probes = self.checked_probes(shape, probes)
        self.regions = self.checked_regions(shape, regions)
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("CylFieldMonitor: capacity must be >= 1")
        self.grid, self.capacity = grid, capacity
        self._d_extra = None
        if extra is not None:
            self._d_extra = _native_f64(grid, extra, "CylFieldMonitor: extra must be an fp64 device field in the grid's layout")
        nreg, npr = len(self.regions), len(self.probes)
        self.row_words = npr + self.REGION_WORDS * nreg
        self._h_regions = (ctypes.c_int * (6 * nreg))(*[v for box in self.regions for ax in box for v in ax])
        self._h_probes = (ctypes.c_int * (3 * npr))(*[v for p in self.probes for v in p]) if npr else None
        self._d_probes = torch.tensor([v for p in self.probes for v in p], dtype=torch.int32, device=_device()) if npr else None
        self.d_partial = torch.zeros(self.partial_words(shape, self.regions), dtype=torch.int64, device=_device())
        words = (capacity + 1) * self.row_words
        self._log_store = torch.full((words + 2 * self.LOG_GUARD,), self.GUARD_WORD, dtype=torch.int64, device=_device())
        self.d_log = self._log_store[self.LOG_GUARD:self.LOG_GUARD + words]
        self.d_block = torch.zeros(_lib.HISTORY_BLOCK_BYTES // 8, dtype=torch.int64, device=_device())
        self._d_act = None           # the active mask of the step being recorded (the step sets it around _record_step)
        self.reset(t)

    # -- arguments (no device needed) ----------------------------------------------------------------------------------------
    @staticmethod
    def checked_probes(shape, probes):
        """the probes as a tuple of (i, j, k); ValueError for more than 256 of them or one outside the grid `shape`"""
        out = []
        for p in probes:
            p = tuple(p)
            if len(p) != 3 or any(int(v) != v for v in p):
                raise ValueError("CylFieldMonitor: a probe is a cell (i, j, k), got %r" % (p,))
            p = tuple(int(v) for v in p)
            if any(not 0 <= v < n for v, n in zip(p, shape)):
                raise ValueError("CylFieldMonitor: probe %r lies outside the grid %r" % (p, tuple(shape)))
            out.append(p)
        if len(out) > CylFieldMonitor.MAX_PROBES:
            raise ValueError("CylFieldMonitor: %d probes (at most %d)" % (len(out), CylFieldMonitor.MAX_PROBES))
        return tuple(out)

    @staticmethod
    def checked_regions(shape, regions):
        """the regions as a tuple of ((i0, i1), (j0, j1), (k0, k1)), None entries (and no entry at all) as the whole grid;
        ValueError for more than 8, an empty one, one that leaves the grid along r or z, or a phi range outside
        0 <= j0 < nphi, j0 < j1 <= j0 + nphi"""
        nr, nphi, nz = (int(n) for n in shape)
        whole = ((0, nr), (0, nphi), (0, nz))
        if regions is None or len(regions) == 0:
            regions = (None,)
        out = []
        for box in regions:
            if box is None:
                out.append(whole)
                continue
            box = tuple(tuple(ax) for ax in box)
            if len(box) != 3 or any(len(ax) != 2 or any(int(v) != v for v in ax) for ax in box):
                raise ValueError("CylFieldMonitor: a region is ((i0, i1), (j0, j1), (k0, k1)), got %r" % (box,))
            box = tuple((int(lo), int(hi)) for lo, hi in box)
            if any(lo >= hi for lo, hi in box):
                raise ValueError("CylFieldMonitor: region %r is empty" % (box,))
            (i0, i1), (j0, j1), (k0, k1) = box
            if i0 < 0 or i1 > nr or k0 < 0 or k1 > nz or not 0 <= j0 < nphi or j1 > j0 + nphi:
                raise ValueError("CylFieldMonitor: region %r leaves the grid %r (phi: 0 <= j0 < nphi, j1 <= j0 + nphi)"
                                 % (box, (nr, nphi, nz)))
            out.append(box)
        if len(out) > CylFieldMonitor.MAX_REGIONS:
            raise ValueError("CylFieldMonitor: %d regions (1 to %d)" % (len(out), CylFieldMonitor.MAX_REGIONS))
        return tuple(out)

    @staticmethod
    def cells_of(grid, points):
        """points (r, phi, z) -> cells: i = floor((r - R_in)/dr), j = floor(phi/dphi) mod nphi (any real phi),
        k = floor(z/dz); ValueError for r or z outside the grid"""
        out = []
        for pt in points:
            r, phi, z = (float(v) for v in pt)
            i = int(math.floor((r - grid.R_in) / grid.dr))
            j = int(math.floor(phi / grid.dphi)) % grid.nphi
            k = int(math.floor(z / grid.dz))
            if not (0 <= i < grid.nr and 0 <= k < grid.nz):
                raise ValueError("CylFieldMonitor.cells_of: point %r lies outside the grid" % (tuple(pt),))
            out.append((i, j, k))
        return tuple(out)

    @staticmethod
    def chunks(shape):
        """(per_line, nchunk) of a plane: pairs per phi line, chunks of 256 pairs per plane"""
        per_line = -(-int(shape[2]) // 2)
        return per_line, -(-int(shape[1]) * per_line // 256)

    @staticmethod
    def partial_words(shape, regions):
        """8-byte words of the partial buffer: ADI_CYL_MONITOR_PARTIAL_WORDS per (region, radius, chunk) and (region, radius)"""
        nchunk = CylFieldMonitor.chunks(shape)[1]
        return _lib.CYL_MONITOR_PARTIAL_WORDS * sum((i1 - i0) * (nchunk + 1) for (i0, i1), _, _ in regions)

    @staticmethod
    def rounding_depth(shape, box):
        """d of the definition for this region: 19 + ceil(nchunk / 256) + (i1 - i0); one more for the r-weighted sums"""
        nchunk = CylFieldMonitor.chunks(shape)[1]
        return 19 + -(-nchunk // 256) + (box[0][1] - box[0][0])

    @staticmethod
    def region_cells(shape, box):
        """the cells of a region as a bool array: the phi range taken mod nphi"""
        (i0, i1), (j0, j1), (k0, k1) = box
        inc = np.zeros(shape, dtype=bool)
        inc[i0:i1, np.arange(j0, j1) % shape[1], k0:k1] = True
        return inc

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def plane_sums(V):
        """S_i of every plane of V (the grid's shape, +0.0 on every excluded cell) in THE ORDER of the monitor"""
        nr, nphi, nz = V.shape
        per_line, nchunk = CylFieldMonitor.chunks(V.shape)
        P = np.zeros((nr, nphi, 2 * per_line))             # the missing partner of an odd nz: +0.0
        P[:, :, :nz] = V
        pair = P[:, :, 0::2] + P[:, :, 1::2]
        padded = np.zeros((nr, nchunk * 256))              # +0.0 past the last pair
        padded[:, :nphi * per_line] = pair.reshape(nr, -1)
        partial = FieldMonitor._waves(padded.reshape(nr, nchunk, 256))
        # the plane's workgroup: thread t adds the partials t, t + 256, ... in increasing order, from +0.0
        rows = -(-nchunk // 256)
        padded = np.zeros((nr, rows * 256))
        padded[:, :nchunk] = partial
        acc = np.zeros((nr, 256))
        for n in range(rows):
            acc = acc + padded[:, 256 * n:256 * (n + 1)]
        return FieldMonitor._waves(acc)

    @staticmethod
    def record_reference(T, active, probes, regions, grid, extra=None):
        """One row of the log from the field T: THE DEFINITION of the monitor -- one fp64 operation per line, in the order the
        kernels perform them.  active: bool array (None: every cell); grid: a GridCyl or (R_in, dr).
        -> dict(probes, cells, sum_i, T_min, T_max, sum_T, sum_rT, sum_extra, sum_rextra): `probes` one value per probe, T at
        the cell, NaN where it is not active; the others one value per region over its active cells (sum_extra and sum_rextra
        +0.0 without `extra`; a NaN of `extra` on an included cell contributes +0.0).

        The order of a sum depends on the grid's shape, on (R_in, dr) and on the region's box, on nothing else.  An excluded
        cell -- inactive, outside the region, the missing partner of an odd nz -- contributes +0.0.
          plane   of radius i: per_line = ceil(nz/2); pair q = j*per_line + p holds the cells (j, 2p), (j, 2p + 1):
                  pair = v0 + v1.  Chunk c holds the pairs 256c .. 256c + 255, one per thread, +0.0 past the last pair.  A wave
                  of 64 threads: v = v + v[lane ^ o] for o = 1, 2, 4, 8, 16, 32.  The four waves: ((w0 + w1) + w2) + w3:
                  partial[i][c].  Over the nchunk = ceil(nphi*per_line/256) partials, thread t of 256: acc = +0.0;
                  acc = acc + partial[i][n] for n = t, t + 256, ...; the same butterfly and wave order: S_i.
          region  sum_T: acc = +0.0; acc = acc + S_i for i = i0 .. i1 - 1.  sum_rT: p = r_i * S_i first, one operation, then
                  acc = acc + p, with r_i = R_in + (i + 0.5)*dr as GridCyl.r computes it.
        d, the rounding operations on the longest path from a cell to the logged sum: 1 + 6 + 3 in the chunk,
        ceil(nchunk/256) + 6 + 3 in the plane, i1 - i0 in the region: d = 19 + ceil(nchunk/256) + (i1 - i0)
        (`rounding_depth`); d + 1 for the r-weighted sums.  So |sum - exact| <= d eps sum|terms|, eps = 2^-52.
        T_min, T_max: the extrema in the order of the finite doubles with -0.0 < +0.0, NaN when the region has no active
        cell; the rules of FieldMonitor.record_reference.  Precondition: no NaN on active cells."""
        T = np.asarray(T, dtype=np.float64)
        act = np.ones(T.shape, dtype=bool) if active is None else np.asarray(active, dtype=bool)
        regions = CylFieldMonitor.checked_regions(T.shape, regions)
        probes = CylFieldMonitor.checked_probes(T.shape, probes)
        R_in, dr = (grid.R_in, grid.dr) if hasattr(grid, 'dr') else grid
        r = float(R_in) + (np.arange(T.shape[0], dtype=np.float64) + 0.5) * float(dr)
        out = dict(probes=np.array([T[p] if act[p] else np.nan for p in probes], dtype=np.float64))
        fields = {'sum_T': T}
        if extra is not None:
            X = np.asarray(extra, dtype=np.float64)
            fields['sum_extra'] = np.where(np.isnan(X), 0.0, X)
        rows = {k: [] for k in CylFieldMonitor.NAMES}
        for box in regions:
            inc = CylFieldMonitor.region_cells(T.shape, box) & act
            (i0, i1) = box[0]
            vals = T[inc]
            rows['cells'].append(int(vals.size))
            rows['sum_i'].append(int(np.argwhere(inc)[:, 0].sum()))
            if vals.size:
                lo, hi = vals.min(), vals.max()
                zeros = vals[vals == 0.0]
                if lo == 0.0:
                    lo = -0.0 if np.signbit(zeros).any() else 0.0
                if hi == 0.0:
                    hi = 0.0 if (~np.signbit(zeros)).any() else -0.0
            else:
                lo = hi = np.nan
            rows['T_min'].append(lo)
            rows['T_max'].append(hi)
            for name, rname in (('sum_T', 'sum_rT'), ('sum_extra', 'sum_rextra')):
                F = fields.get(name)
                acc, racc = 0.0, 0.0
                if F is not None:
                    S = CylFieldMonitor.plane_sums(np.where(inc, F, 0.0))
                    for i in range(i0, i1):
                        acc = acc + S[i]
                        p = r[i] * S[i]
                        racc = racc + p
                rows[name].append(float(acc))
                rows[rname].append(float(racc))
        for name in ('cells', 'sum_i'):
            out[name] = np.array(rows[name], dtype=np.int64)
        for name in CylFieldMonitor.NAMES[2:]:
            out[name] = np.array(rows[name], dtype=np.float64)
        return out

    @staticmethod
    def row_of(ref):
        """the 8-byte words of a log row from record_reference's dict, as int64 bit patterns"""
        nreg = len(ref['cells'])
        reg = np.empty((nreg, CylFieldMonitor.REGION_WORDS), dtype=np.int64)
        reg[:, 0], reg[:, 1] = ref['cells'], ref['sum_i']
        for q, name in enumerate(CylFieldMonitor.NAMES[2:]):
            reg[:, 2 + q] = np.asarray(ref[name], dtype=np.float64).view(np.int64)
        return np.concatenate([np.asarray(ref['probes'], dtype=np.float64).view(np.int64), reg.ravel()])

    # -- the device side -------------------------------------------------------------------------------------------------------
    def _launch_record(self, t_in, t_out):
        """adi_cyl_monitor_record on t_out (t_in: the step's input, not read) over the cells of _d_act, and the tick of the block"""
        g = self.grid
        check(lib.adi_cyl_monitor_record(_p(self.d_block), _p(t_out), _p(self._d_extra), _p(self._d_act), *g.layout.pd,
                                         g.R_in, g.dr, len(self.regions), self._h_regions, len(self.probes), self._h_probes,
                                         _p(self._d_probes), _p(self.d_partial), self.d_partial.numel(), _p(self.d_log),
                                         self.capacity, _stream()))
        check(lib.adi_history_tick(_p(self.d_block), _stream()))

    def _check_mask(self):
        """(stateless: every mask is the right one)"""

    def record(self, T_out, dt, active=None):
        """one row from T_out, an fp64 device field in the grid's layout, over the cells of `active` (None: all) at the log's
        slot, and the tick; afterwards .t = .t + dt.  dt = 0.0 logs a state without moving the clock: record(T0, 0.0) for the
        initial one"""
        t_out = _native_f64(self.grid, T_out, "CylFieldMonitor.record: T_out must be an fp64 device field in the grid's layout")
        dt = float(dt)
        if not (np.isfinite(dt) and dt >= 0.0):
            raise ValueError("CylFieldMonitor.record: dt must be finite and >= 0")
        self._d_act = _active_arg(self.grid, active)
        try:
            self._launch_record(None, t_out)
        finally:
            self._d_act = None
        self.advance_clock(self.t, dt, 1)

    def _record_step(self, t_in, out, dt, captured, d_act=None):
        """what the step calls for "record this step" on its final field `out` over the cells of d_act (None: all).  captured:
        the record and the tick alone, the caller keeps the clock; otherwise `record`"""
        if not captured:
            return self.record(out, dt, active=d_act)
        self._d_act = d_act
        try:
            self._launch_record(t_in, out)
        finally:
            self._d_act = None

    def reset(self, t=0.0):
        """the log empty (slot 0), .t = t"""
        check(lib.adi_cyl_monitor_reset_log(_p(self.d_block), _p(self.d_log), self.capacity, self.row_words, _stream()))
        self._times = []
        self.t = float(t)

    snapshot = FieldMonitor.snapshot
    restore = FieldMonitor.restore
    slot = FieldMonitor.slot
    guards = FieldMonitor.guards
    rows = FieldMonitor.rows
    traces = FieldMonitor.traces

    def graph_key(self):
        """what a captured graph holds of the monitor: probes, regions and (R_in, dr) by value, the buffers by pointer"""
        return (self.probes, self.regions, self.grid.R_in, self.grid.dr,
                None if self._d_extra is None else self._d_extra.data_ptr(), self.d_partial.data_ptr(), self.d_log.data_ptr(),
                self.d_block.data_ptr(), None if self._d_probes is None else self._d_probes.data_ptr())

    def region_log(self, mat=None):
        """the log of the regions as arrays [region, step]: cells, sum_i (int64), T_min, T_max, sum_T, sum_rT,
        T_mean = sum_T / cells, volume = CylThermalHistory.pool_volume(grid, cells, sum_i) (exact),
        T_vmean = sum_rT / ((R_in + dr/2) cells + dr sum_i), heat = (rho cp)(dr dphi dz) sum_rT for the `mat` given (absent
        without one), and with `extra`: sum_extra, sum_rextra and extra_volume = dr dphi dz sum_rextra (the molten volume when
        `extra` is a liquid fraction); with t (the end time of every recorded step) and dropped"""
        rows, dropped = self.rows()
        g, nreg, npr, rw = self.grid, len(self.regions), len(self.probes), self.REGION_WORDS
        reg = rows[:, npr:].reshape(len(rows), nreg, rw).transpose(1, 0, 2)
        f = lambda q: reg[:, :, q].copy().view(np.float64)      # noqa: E731
        cells, sum_i, sum_T, sum_rT = reg[:, :, 0].copy(), reg[:, :, 1].copy(), f(4), f(5)
        cell = g.dr * g.dphi * g.dz
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = sum_T / cells
            vmean = sum_rT / ((g.R_in + 0.5 * g.dr) * cells.astype(np.float64) + g.dr * sum_i.astype(np.float64))
        out = dict(t=np.asarray(self._times[:len(rows)], dtype=np.float64), cells=cells, sum_i=sum_i, T_min=f(2), T_max=f(3),
                   sum_T=sum_T, sum_rT=sum_rT, T_mean=mean, volume=CylThermalHistory.pool_volume(g, cells, sum_i),
                   T_vmean=vmean, dropped=dropped)
        if mat is not None:
            out['heat'] = (mat.rho * mat.cp) * cell * sum_rT
        if self._d_extra is not None:
            out.update(sum_extra=f(6), sum_rextra=f(7), extra_volume=cell * f(7))
        return out
