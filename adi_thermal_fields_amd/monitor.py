"""The field monitor of the Cartesian step, `FieldMonitor`: probe temperatures, the extrema and the sums of index boxes, one
row of a device log per recorded step (include/adi_hip.h, "Field monitor")."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .fields import DeviceField, _device, _native_f64, _p, _stream
from .packs import MaterialMap
from .history import _StepRecorder

_B = _lib.BRICK
_LANES = np.arange(64)


class FieldMonitor(_StepRecorder):
    """What a run is calibrated and checked with, logged on the device after every recorded step: the step's final field at
    up to 256 `probes` (cells (i, j, k) of the logical grid; NaN while the cell is off the mask) and, over the in-mask cells of
    1 to 8 `regions` (half-open index boxes ((i0, i1), (j0, j1), (k0, k1)) inside the logical box, None: the whole grid, also
    what an empty `regions` means; they may overlap): `cells`, `T_min`, `T_max` (NaN when cells == 0), `sum_T`, with
    `material_map` (a MaterialMap of the grid) `sum_wT`, the sum of w[id]*T with w[m] = (rho_m cp_m) dx**3 computed on the host
    and passed by value, and with `extra` (an fp64 device field in the grid's layout, held by pointer: the liquid fraction of a
    PhaseField, say) `sum_extra`.  The log has `capacity` rows and a spill row; the block and the host clock `.t` are the
    thermal history's.  The monitor holds no per-cell state: it reads the grid's flags and their summary as they are, so a mask
    change (a birth, a deposit) needs no call.
        record(T_out, dt)         one row from T_out at the block's slot, then the tick; record(T0, 0.0) logs the initial state
        reset(t=0.0)              the log empty (slot 0), .t = t
        snapshot() / restore(s)   the log, the block and the host clock
        traces()                  t and T[probe, step]
        region_log(mat=None)      t, cells, T_min, T_max, T_mean, sum_T, heat, sum_extra (arrays [region, step]) and dropped
    `record_reference` is the definition, adi_monitor_record the same operations on the device.
    Not covered: SlabStepper and the adi_ctx_* API (the cylindrical step has CylFieldMonitor, cyl_monitor.py); probes between cell centres; where the extremum lies;
    regions given by a label field; control loops that read the log."""

    LOG_GUARD = 8        # 8-byte words either side of the log that no launch may touch (tests read them)
    GUARD_WORD = 0x5a5a5a5a5a5a5a5a
    MAX_PROBES = _lib.MONITOR_MAX_PROBES
    MAX_REGIONS = _lib.MONITOR_MAX_REGIONS
    _keyword = 'monitor'

    def __init__(self, grid, probes=(), regions=(), capacity=4096, material_map=None, extra=None, t=0.0):
        shape = tuple(grid.shape)
        self.probes = self.checked_probes(shape, probes)
        self.regions = self.checked_regions(shape, regions)
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("FieldMonitor: capacity must be >= 1")
        if material_map is not None:
            if not isinstance(material_map, MaterialMap):
                raise TypeError("FieldMonitor: material_map must be a MaterialMap")
            if material_map.grid is not grid:
                raise ValueError("FieldMonitor: the MaterialMap belongs to another grid")
        self.grid, self.capacity, self.material_map = grid, capacity, material_map
        self._d_extra = None
        if extra is not None:
            self._d_extra = _native_f64(grid, extra, "FieldMonitor: extra must be an fp64 device field in the grid's layout")
        self.weights = None if material_map is None else self.weights_of(material_map.materials, grid.dx)
        nreg, npr = len(self.regions), len(self.probes)
        self.row_words = npr + _lib.MONITOR_REGION_WORDS * nreg
        self._h_regions = (ctypes.c_int * (6 * nreg))(*[v for box in self.regions for ax in box for v in ax])
        self._h_probes = (ctypes.c_int * (3 * npr))(*[v for p in self.probes for v in p]) if npr else None
        self._h_weights = None if self.weights is None else (ctypes.c_double * len(self.weights))(*self.weights)
        self._d_probes = torch.tensor([v for p in self.probes for v in p], dtype=torch.int32, device=_device()) if npr else None
        records = sum(self.brick_count(box) for box in self.regions)
        self.d_partial = torch.zeros(records * _lib.MONITOR_PARTIAL_WORDS, dtype=torch.int64, device=_device())
        words = (capacity + 1) * self.row_words
        self._log_store = torch.full((words + 2 * self.LOG_GUARD,), self.GUARD_WORD, dtype=torch.int64, device=_device())
        self.d_log = self._log_store[self.LOG_GUARD:self.LOG_GUARD + words]
        self.d_block = torch.zeros(_lib.HISTORY_BLOCK_BYTES // 8, dtype=torch.int64, device=_device())
        self.reset(t)

    # -- arguments (no device needed) ----------------------------------------------------------------------------------------
    @staticmethod
    def checked_probes(shape, probes):
        """the probes as a tuple of (i, j, k); ValueError for more than 256 of them or one outside the box `shape`"""
        out = []
        for p in probes:
            p = tuple(p)
            if len(p) != 3 or any(int(v) != v for v in p):
                raise ValueError("FieldMonitor: a probe is a cell (i, j, k), got %r" % (p,))
            p = tuple(int(v) for v in p)
            if any(not 0 <= v < n for v, n in zip(p, shape)):
                raise ValueError("FieldMonitor: probe %r lies outside the grid %r" % (p, tuple(shape)))
            out.append(p)
        if len(out) > FieldMonitor.MAX_PROBES:
            raise ValueError("FieldMonitor: %d probes (at most %d)" % (len(out), FieldMonitor.MAX_PROBES))
        return tuple(out)

    @staticmethod
    def checked_regions(shape, regions):
        """the regions as a tuple of ((i0, i1), (j0, j1), (k0, k1)), None entries (and no entry at all) as the whole box;
        ValueError for more than 8, an empty one or one that leaves the box `shape`"""
        whole = tuple((0, int(n)) for n in shape)
        if regions is None or len(regions) == 0:
            regions = (None,)
        out = []
        for box in regions:
            if box is None:
                out.append(whole)
                continue
            box = tuple(tuple(ax) for ax in box)
            if len(box) != 3 or any(len(ax) != 2 or any(int(v) != v for v in ax) for ax in box):
                raise ValueError("FieldMonitor: a region is ((i0, i1), (j0, j1), (k0, k1)), got %r" % (box,))
            box = tuple((int(lo), int(hi)) for lo, hi in box)
            if any(lo >= hi for lo, hi in box):
                raise ValueError("FieldMonitor: region %r is empty" % (box,))
            if any(lo < 0 or hi > n for (lo, hi), n in zip(box, shape)):
                raise ValueError("FieldMonitor: region %r leaves the grid %r" % (box, tuple(shape)))
            out.append(box)
        if len(out) > FieldMonitor.MAX_REGIONS:
            raise ValueError("FieldMonitor: %d regions (1 to %d)" % (len(out), FieldMonitor.MAX_REGIONS))
        return tuple(out)

    @staticmethod
    def cells_of(grid, points, origin=(0.0, 0.0, 0.0)):
        """points in metres -> cells: floor((x - origin) / dx) per axis; ValueError for a point outside the box"""
        out = []
        for pt in points:
            cell = tuple(int(math.floor((float(x) - float(o)) / grid.dx)) for x, o in zip(pt, origin))
            if len(cell) != 3 or any(not 0 <= c < n for c, n in zip(cell, grid.shape)):
                raise ValueError("FieldMonitor.cells_of: point %r lies outside the grid" % (tuple(pt),))
            out.append(cell)
        return tuple(out)

    @staticmethod
    def weights_of(materials, dx):
        """the per-material weight of sum_wT: w[m] = (rho_m cp_m) dx**3, two products of fp64"""
        V = float(dx) ** 3
        return tuple((float(m.rho) * float(m.cp)) * V for m in materials)

    @staticmethod
    def brick_box(box):
        """(first brick, bricks) per axis of the 16^3 bricks a region meets"""
        return tuple((lo // _B, (hi - 1) // _B - lo // _B + 1) for lo, hi in box)

    @staticmethod
    def brick_count(box):
        return int(np.prod([n for _, n in FieldMonitor.brick_box(box)]))

    @staticmethod
    def rounding_depth(box):
        """d of the definition for this region: 17 + ceil(nb / 256) + 9, nb the bricks of its brick box"""
        return 17 + -(-FieldMonitor.brick_count(box) // 256) + 9

    # -- the definition ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _butterfly(v):
        """the 64 lanes (last axis) of a wave after v = v + v[lane ^ o], o = 1, 2, 4, 8, 16, 32: every lane the same bits"""
        for o in (1, 2, 4, 8, 16, 32):
            v = v + v[..., _LANES ^ o]
        return v

    @staticmethod
    def _waves(v):
        """256 threads (last axis) -> the workgroup's sum: the butterfly in each wave, then ((w0 + w1) + w2) + w3"""
        w = FieldMonitor._butterfly(v.reshape(v.shape[:-1] + (4, 64)))[..., 0]
        s = w[..., 0] + w[..., 1]
        s = s + w[..., 2]
        return s + w[..., 3]

    @staticmethod
    def ordered_sum(V, box):
        """the sum of V (the grid's shape, +0.0 on every excluded cell) over `box` in THE ORDER of the monitor"""
        (b0, n0), (b1, n1), (b2, n2) = FieldMonitor.brick_box(box)
        P = np.zeros((n0 * _B, n1 * _B, n2 * _B))        # the region's brick box; +0.0 outside the region and the grid
        sl = tuple(slice(lo, hi) for lo, hi in box)
        P[tuple(slice(lo - b * _B, hi - b * _B) for (lo, hi), b in zip(box, (b0, b1, b2)))] = V[sl]
        # local (i, j, k) = (2 g + ih, jl, 2 kp + s) of row group g is thread ih*128 + jl*8 + kp
        v = P.reshape(n0, 8, 2, n1, 16, n2, 8, 2).transpose(0, 3, 5, 1, 2, 4, 6, 7)
        pair = v[..., 0] + v[..., 1]
        acc = pair[:, :, :, 0]
        for g in range(1, 8):
            acc = acc + pair[:, :, :, g]
        bricks = FieldMonitor._waves(acc.reshape(n0, n1, n2, 256)).ravel()      # lexicographic (bi, bj, bk)
        # the finishing workgroup: thread t adds the bricks t, t + 256, ... in increasing order, from +0.0
        rows = -(-bricks.size // 256)
        padded = np.zeros(rows * 256)
        padded[:bricks.size] = bricks
        acc = np.zeros(256)
        for row in padded.reshape(rows, 256):
            acc = acc + row                               # (a thread past the last brick adds +0.0 to a value that is never
        return float(FieldMonitor._waves(acc))            # -0.0: the same bits as not adding)

    @staticmethod
    def record_reference(T, mask, probes, regions, weights=None, ids=None, extra=None):
        """One row of the log from the field T: THE DEFINITION of the monitor -- one fp64 operation per line, in the order the
        kernels perform them.  -> dict(probes, cells, T_min, T_max, sum_T, sum_wT, sum_extra): `probes` one value per probe, T
        at the cell, NaN where it is off the mask; the others one value per region over its in-mask cells (sum_wT and sum_extra
        0.0 without `weights` / `extra`).

        The order of a sum depends on the decomposition of the grid into 16^3 bricks (from the origin) and on the region's box,
        on nothing else.  An excluded cell -- off the mask, outside the region, outside the grid -- contributes +0.0.
          brick   thread t of 256 owns, in row groups g = 0 .. 7, the pair of cells local (i, j, k) = (2 g + (t >> 7),
                  (t >> 3) & 15, 2 (t & 7) + {0, 1}):  pair_g = v0 + v1;  acc = pair_0;  acc = acc + pair_g, g = 1 .. 7.
                  A wave of 64 threads: v = v + v[lane ^ o] for o = 1, 2, 4, 8, 16, 32.  The four waves: ((w0 + w1) + w2) + w3.
          region  its bricks numbered lexicographically (bi, bj, bk) over its brick box; thread t of 256: acc = +0.0;
                  acc = acc + brick[n] for n = t, t + 256, ... ; then the same wave butterfly and the same wave order.
        sum_wT: the product p = w[id] * T is formed first, one operation, then p is summed like T.
        d, the rounding operations on the longest path from a cell to the logged sum: 1 + 7 + 6 + 3 = 17 in the brick,
        ceil(nb / 256) + 6 + 3 in the region, nb the bricks of its brick box: d = 17 + ceil(nb / 256) + 9 (`rounding_depth`);
        d + 1 for sum_wT.  So |sum - exact| <= d eps sum|terms|, eps = 2^-52.
        T_min, T_max: the extrema in the order of the finite doubles with -0.0 < +0.0 -- among zeros T_min is -0.0 if any
        in-mask cell of the region holds -0.0, T_max is +0.0 if any holds +0.0 -- so they depend on no order of evaluation.  NaN
        when the region has no in-mask cell.  Precondition: no NaN on in-mask cells."""
        T = np.asarray(T, dtype=np.float64)
        m = np.asarray(mask, dtype=bool)
        regions = FieldMonitor.checked_regions(T.shape, regions)
        probes = FieldMonitor.checked_probes(T.shape, probes)
        out = dict(probes=np.array([T[p] if m[p] else np.nan for p in probes], dtype=np.float64))
        fields = {'sum_T': T}
        if weights is not None:
            w = np.zeros(8)
            w[:len(weights)] = weights
            with np.errstate(invalid='ignore', over='ignore'):
                wT = w[np.asarray(ids).astype(np.intp) & 7] * T      # (off the mask the product is formed and never used)
            fields['sum_wT'] = wT
        if extra is not None:
            fields['sum_extra'] = np.asarray(extra, dtype=np.float64)
        rows = {k: [] for k in ('cells', 'T_min', 'T_max', 'sum_T', 'sum_wT', 'sum_extra')}
        for box in regions:
            inc = np.zeros(T.shape, dtype=bool)
            sl = tuple(slice(lo, hi) for lo, hi in box)
            inc[sl] = m[sl]
            vals = T[inc]
            rows['cells'].append(int(vals.size))
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
            for name in ('sum_T', 'sum_wT', 'sum_extra'):
                F = fields.get(name)
                rows[name].append(0.0 if F is None else FieldMonitor.ordered_sum(np.where(inc, F, 0.0), box))
        out['cells'] = np.array(rows['cells'], dtype=np.int64)
        for name in ('T_min', 'T_max', 'sum_T', 'sum_wT', 'sum_extra'):
            out[name] = np.array(rows[name], dtype=np.float64)
        return out

    @staticmethod
    def row_of(ref):
        """the 8-byte words of a log row from record_reference's dict, as int64 bit patterns"""
        nreg = len(ref['cells'])
        reg = np.empty((nreg, _lib.MONITOR_REGION_WORDS), dtype=np.int64)
        reg[:, 0] = ref['cells']
        for q, name in enumerate(('T_min', 'T_max', 'sum_T', 'sum_wT', 'sum_extra')):
            reg[:, 1 + q] = np.asarray(ref[name], dtype=np.float64).view(np.int64)
        return np.concatenate([np.asarray(ref['probes'], dtype=np.float64).view(np.int64), reg.ravel()])

    # -- the device side -------------------------------------------------------------------------------------------------------
    def _launch_record(self, t_in, t_out):
        """adi_monitor_record on t_out (t_in: the step's input, not read) and the tick of the block"""
        g, mm = self.grid, self.material_map
        check(lib.adi_monitor_record(_p(self.d_block), _p(t_out), _p(self._d_extra), _p(None if mm is None else mm._d_ids),
                                     _p(g.d_flags), _p(g.d_bricks), *g.layout.pd, len(self.regions), self._h_regions,
                                     len(self.probes), self._h_probes, _p(self._d_probes),
                                     0 if mm is None else len(mm.materials), self._h_weights, _p(self.d_partial),
                                     self.d_partial.numel(), _p(self.d_log), self.capacity, _stream()))
        check(lib.adi_history_tick(_p(self.d_block), _stream()))

    def _check_mask(self):
        """(stateless: every mask is the right one)"""

    def record(self, T_out, dt, T_in=None):
        """one row from T_out, an fp64 device field in the grid's layout, at the log's slot, and the tick; afterwards
        .t = .t + dt.  dt = 0.0 logs a state without moving the clock: record(T0, 0.0) for the initial one"""
        t_out = _native_f64(self.grid, T_out, "FieldMonitor.record: T_out must be an fp64 device field in the grid's layout")
        dt = float(dt)
        if not (np.isfinite(dt) and dt >= 0.0):
            raise ValueError("FieldMonitor.record: dt must be finite and >= 0")
        self._launch_record(None, t_out)
        self.advance_clock(self.t, dt, 1)

    def _record_step(self, t_in, out, dt, captured):
        if captured:
            self._launch_record(t_in, out)
        else:
            self.record(out, dt)                              # (its own signature: the non-captured half differs)

    def reset(self, t=0.0):
        """the log empty (slot 0), .t = t"""
        check(lib.adi_monitor_reset_log(_p(self.d_block), _p(self.d_log), self.capacity, self.row_words, _stream()))
        self._times = []
        self.t = float(t)

    def snapshot(self):
        return self._log_store.clone(), self.d_block.clone(), self.t, list(self._times)

    def restore(self, s):
        self._log_store.copy_(s[0])
        self.d_block.copy_(s[1])
        self.t = s[2]
        self._times = list(s[3])

    def graph_key(self):
        """what a captured graph holds of the monitor: probes, regions and weights by value, the buffers by pointer"""
        mm = self.material_map
        return (self.probes, self.regions, self.weights, None if mm is None else mm.graph_key(),
                None if self._d_extra is None else self._d_extra.data_ptr(), self.d_partial.data_ptr(), self.d_log.data_ptr(),
                self.d_block.data_ptr(), None if self._d_probes is None else self._d_probes.data_ptr())

    @property
    def slot(self):
        """rows recorded since the last reset (read from the device block)"""
        return int(self.d_block.cpu()[3].item())

    def guards(self):
        """the guard words below and above the log, as NumPy int64"""
        s = self._log_store.cpu().numpy()
        return s[:self.LOG_GUARD].copy(), s[-self.LOG_GUARD:].copy()

    def rows(self):
        """the recorded rows as int64 bit patterns, (n, row_words), and the number of rows dropped past the capacity"""
        slot = self.slot
        n = min(slot, self.capacity)
        return self.d_log.cpu().numpy().reshape(self.capacity + 1, self.row_words)[:n].copy(), max(0, slot - self.capacity)

    def traces(self):
        """dict(t, T): the end time of every recorded step and T[probe, step], NaN while the probe's cell is off the mask"""
        rows, _ = self.rows()
        return dict(t=np.asarray(self._times[:len(rows)], dtype=np.float64),
                    T=rows[:, :len(self.probes)].view(np.float64).T.copy())

    def region_log(self, mat=None):
        """the log of the regions as arrays [region, step]: cells (int64), T_min, T_max, T_mean = sum_T / cells, sum_T, heat,
        sum_extra (only with `extra`), with t (the end time of every recorded step) and dropped.  heat = sum_wT with a
        MaterialMap; without one (rho cp dx**3) sum_T for the `mat` given here, and absent when none is given"""
        rows, dropped = self.rows()
        nreg, npr, rw = len(self.regions), len(self.probes), _lib.MONITOR_REGION_WORDS
        reg = rows[:, npr:].reshape(len(rows), nreg, rw).transpose(1, 0, 2)
        f = lambda q: reg[:, :, q].copy().view(np.float64)      # noqa: E731
        cells, sum_T = reg[:, :, 0].copy(), f(3)
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = sum_T / cells
        out = dict(t=np.asarray(self._times[:len(rows)], dtype=np.float64), cells=cells, T_min=f(1), T_max=f(2), T_mean=mean,
                   sum_T=sum_T, dropped=dropped)
        if self.material_map is not None:
            out['heat'] = f(4)
        elif mat is not None:
            out['heat'] = (mat.rho * mat.cp * self.grid.dx ** 3) * sum_T
        if self._d_extra is not None:
            out['sum_extra'] = f(5)
        return out
