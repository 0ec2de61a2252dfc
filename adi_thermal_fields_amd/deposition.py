"""Deposition helpers: the surface impulse, the perimeter ratio of a voxelised section, layer births on the device
(`birth_planes`, `BirthPacks`), and bead-by-bead births along a scan path (`BeadProfile`, `PathDeposit`)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from .fields import DeviceField, Grid3D, _device, _native_f64, _p, _stream
from .heat_source import ScanPath, ScanPathSource
from .packs import AxisCoeffPack, MaterialMap, _face_constants


def apply_surface_impulse_Q(T, grid, mat, Q, face='z-'):
    """adi3d_numba_coeff.py:304-320: add dT = Q/(rho cp dx) to the in-mask cells of the domain-boundary plane of
    `face`, IN PLACE (NumPy array or DeviceField).  ValueError("bad face") for an unknown face."""
    if face not in FACES:
        raise ValueError("bad face")
    dT = Q / (mat.rho * mat.cp * grid.dx)
    ax, plus = FACES.index(face) // 2, FACES.index(face) % 2
    sl = [slice(None)] * 3
    sl[ax] = -1 if plus else 0
    sl = tuple(sl)
    if isinstance(T, DeviceField):
        sel = (grid.d_mask[sl] != 0)
        plane = T.t[sl]
        plane[sel] = plane[sel] + dT
    else:
        sel = np.asarray(grid.mask)[sl]
        T[sl][sel] += dT


# ---- per-voxel Robin correction: perimeter ratio --------------------------------------------
_LATERAL = ('x-', 'x+', 'y-', 'y+')


def exposed_faces_per_layer(mask_or_grid, faces=_LATERAL):
    """Number of exposed faces (in-mask cell whose neighbour across the face is outside the mask or the box) per plane
    k of axis 2, counted on the device from the neighbour-flags digest: int64 array of length nz.  With the four
    lateral faces this is the digital perimeter of every layer divided by dx."""
    for f in faces:
        if f not in FACES:
            raise ValueError("bad face")
    if isinstance(mask_or_grid, Grid3D):
        g = mask_or_grid
    else:
        m = np.asarray(mask_or_grid)
        g = Grid3D(m.shape[0], m.shape[1], m.shape[2], 1.0, m)
    bits = sum(1 << FACES.index(f) for f in set(faces))
    counts = torch.empty(g.layout.pz, dtype=torch.int64, device=_device())
    check(lib.adi_count_exposed_faces(_p(g.d_flags), *g.layout.pd, bits, _p(counts), _stream()))
    return counts[:g.nz].cpu().numpy()                # (the planes of the physical box beyond nz hold no in-mask cell)


def count_exposed_faces(mask2d):
    """quick_compare_layer_birth_robin_v3.py:97-108: exposed x-/x+/y-/y+ faces of a 2-D section (an integer)."""
    m = np.asarray(mask2d).astype(bool)
    assert m.ndim == 2
    return int(exposed_faces_per_layer(m[:, :, None])[0])


def perimeter_ratio(mask2d, dx, perim_true):
    """gamma = true perimeter / digital perimeter of the voxelised section (quick_compare_layer_birth_robin_v3.py:109-112);
    the lateral Robin coefficient of a staircase surface is scaled by it: h_side_eff = h_side * gamma (pi/4 for a
    large disk)."""
    faces = count_exposed_faces(mask2d)
    if faces == 0:
        raise ValueError("empty section")
    return float(perim_true) / (faces * float(dx))


# ---- layer birth on the device --------------------------------------------------------------
def birth_planes(T, d_active, d_full, grid, k_begin, k_end, Ts, count=None):
    """activate_layer (waam_from_stl_v7_mm.py:487-495) on the planes [k_begin, k_end) of axis 2, one kernel:
    newborn = full & ~active; T[newborn] = Ts; active |= full.  T: DeviceField; d_active / d_full: uint8 tensors in the
    grid's layout.  `count`: optional int64 device tensor (1 element) that receives the number of newborn cells."""
    L = grid.layout
    assert L.is_native(d_active) and L.is_native(d_full) and L.is_native(T.t)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=T.t.device)
    check(lib.adi_birth_planes(_p(T.t), _p(d_active), _p(d_full), *grid.layout.pd, int(k_begin),
                               int(k_end), float(Ts), _p(count), _stream()))
    return count


class BirthPacks:
    """The coefficient packs of a part that grows by layer births along axis 2 (precompute_coeff_packs_unified with
    scalar / None face specifications, no Dirichlet cells), kept in HBM and UPDATED IN PLACE after a birth: only the
    planes of the new layer and the one below / above it change exposure, so the flags and the six coefficient arrays
    are rebuilt on [k_begin - 1, k_end + 1) instead of the whole box -- the same arrays the reference's full rebuild
    (waam_from_stl_v7_mm.py:534) would give."""

    def __init__(self, grid, mat, robin_h=None, neumann=None):
        self.grid, self.mat = grid, mat
        L = grid.layout

        def spec(v):
            if v is None:
                return (_lib.FACE_NONE, 0.0)
            if not np.isscalar(v):
                raise TypeError("BirthPacks takes scalar face specifications (use precompute_coeff_packs_unified for fields)")
            return (_lib.FACE_SCALAR, float(v))
        hs = [spec(None if robin_h is None else (robin_h.get(f, 0.0) if isinstance(robin_h, dict) else robin_h)) for f in FACES]
        qs = [spec(neumann.get(f) if neumann is not None else None) for f in FACES]
        self._args = ((ctypes.c_int * 6)(*[h[0] for h in hs]), (ctypes.c_double * 6)(*[h[1] for h in hs]), ptr_array([None] * 6),
                      (ctypes.c_int * 6)(*[q[0] for q in qs]), (ctypes.c_double * 6)(*[q[1] for q in qs]), ptr_array([None] * 6))
        self.coeff = [L.empty(zero=True) for _ in range(3)]
        self.qflux = [L.empty(zero=True) for _ in range(3)]
        has_q = any(q[0] != _lib.FACE_NONE for q in qs)
        self.packs = tuple(AxisCoeffPack(self.coeff[a], None, None, self.qflux[a], _has_dir=False, _has_q=has_q, _layout=L)
                           for a in range(3))
        fcs = _face_constants(grid, mat, [h[0] for h in hs], [h[1] for h in hs], [q[0] for q in qs], [q[1] for q in qs])
        for a, p in enumerate(self.packs):
            p.sparse_ok = True
            p.face_consts = fcs[a]
        self.update(0, grid.nz)

    def update(self, k_begin, k_end):
        """rebuild the planes [k_begin, k_end) of axis 2 from the grid's current device mask"""
        g, m = self.grid, self.mat
        k0, k1 = max(0, int(k_begin)), min(g.nz, int(k_end))
        hm, hs, hf, qm, qs, qf = self._args
        check(lib.adi_build_coeffs_planes(_p(g.d_mask), *g.layout.pd, g.dx, m.rho, m.cp, hm, hs, hf, qm, qs, qf,
                                          ptr_array([c.data_ptr() for c in self.coeff]),
                                          ptr_array([q.data_ptr() for q in self.qflux]), k0, k1, _stream()))
        for a, p in enumerate(self.packs):
            p.mask_version = g.mask_version
            p._fractions = (g, a, g.mask_version)
        return self.packs


# ---- bead-by-bead births along a scan path ---------------------------------------------------------------------------
class BeadProfile:
    """The cross-section of the bead a ScanPath lays (README, "Deposition along a path"): `width` across the leg and `height`
    below the path point, which is the TOP of the bead [m]; profile 'box' (the full height over the whole width) or 'parabola'
    (height * (1 - r^2 / (width/2)^2) at distance r from the path).  ValueError for anything else."""
    PROFILES = _lib.BEAD_PROFILES

    def __init__(self, width, height, profile='box'):
        self.width, self.height, self.profile = width, height, profile
        self.validate()

    def validate(self):
        """ValueError for a parameter adi_bead_shape rejects (include/adi_hip.h) -> (width, height) as floats"""
        try:
            w, h = float(self.width), float(self.height)
        except (TypeError, ValueError):
            raise ValueError("BeadProfile: parameters must be real numbers")
        if not (np.isfinite(w) and np.isfinite(h)):
            raise ValueError("BeadProfile: non-finite parameter")
        if min(w, h) <= 0:
            raise ValueError("BeadProfile: non-positive length (width, height must be > 0)")
        if not isinstance(self.profile, str) or self.profile not in self.PROFILES:
            raise ValueError("BeadProfile: profile must be 'box' or 'parabola'")
        return w, h

    def as_c(self, depth_axis):
        w, h = self.validate()
        return _lib.BeadShape(w, h, self.PROFILES[self.profile], int(depth_axis))


class PathDeposit:
    """Material laid where the torch went: the cells a scan path brings to life during a step [t, t + dt] (include/adi_hip.h,
    "Bead deposition along a scan path"; `reference` is the definition).  `path`: a ScanPath, frozen here with on_device(), or a
    ScanPathSource; `bead`: a BeadProfile; newborn cells get T = Ts; `within` (optional bool array or uint8 device tensor of
    the grid's shape): the part's final shape, e.g. from voxelize_solid -- no cell outside it is born.
    The grid's device mask is the active mask: `deposit` writes it in place and rebuilds the grid's flags and bricks on the
    planes whose exposure can have changed; the packs are the caller's (BirthPacks.update / LossPacks.rebuild on the range it
    returns).  Nothing is read back and nothing is synchronised.
    `grid` may also be any object with nx, ny, nz, dx and mask (no device): then `born_host` and `index_box` work, which need
    no GPU, and `deposit` does not.
    material_map, material_id (both or neither): the grid carries several materials (a MaterialMap of this grid) and what this
    path lays is material `material_id` of it: `deposit` also writes that id into the map's device id field on exactly the
    newborn cells (adi_bead_deposit_ids; ids_after = where(reference(...), material_id, ids_before)).  The caller then calls
    `material_map.update(*rng)` on the range `deposit` returns.  One PathDeposit lays one material; use two for two wires."""

    def __init__(self, grid, path, bead, Ts, within=None, material_map=None, material_id=None):
        if isinstance(path, ScanPath):
            path = path.on_device()
        if not isinstance(path, ScanPathSource):
            raise TypeError("PathDeposit: path must be a ScanPath or a ScanPathSource, got %s" % type(path).__name__)
        if not isinstance(bead, BeadProfile):
            raise TypeError("PathDeposit: bead must be a BeadProfile, got %s" % type(bead).__name__)
        try:
            self.Ts = float(Ts)
        except (TypeError, ValueError):
            raise ValueError("PathDeposit: Ts must be a real number")
        if not np.isfinite(self.Ts):
            raise ValueError("PathDeposit: non-finite Ts")
        if (material_map is None) != (material_id is None):
            raise ValueError("PathDeposit: material_map and material_id go together (the map whose id field is stamped, and the "
                             "id of what this path lays)")
        if material_map is not None:
            if not isinstance(material_map, MaterialMap):
                raise TypeError("PathDeposit: material_map must be a MaterialMap, got %s" % type(material_map).__name__)
            if material_map.grid is not grid:
                raise ValueError("PathDeposit: the MaterialMap belongs to another grid")
            if isinstance(material_id, bool) or not isinstance(material_id, (int, np.integer)) \
                    or not 0 <= material_id < len(material_map.materials):
                raise ValueError("PathDeposit: material_id must be an integer from 0 to %d (the MaterialMap has %d materials), "
                                 "got %r" % (len(material_map.materials) - 1, len(material_map.materials), material_id))
            material_id = int(material_id)
        self.material_map, self.material_id = material_map, material_id
        self.grid, self.path, self.bead = grid, path, bead
        self._c_shape = bead.as_c(path.depth_axis)
        self._n = (int(grid.nx), int(grid.ny), int(grid.nz))
        self._on_device = isinstance(grid, Grid3D)
        self._within, self.d_within, self._count = within, None, None
        if within is not None:
            shp = tuple(within.shape) if hasattr(within, 'shape') else np.shape(within)
            if shp != self._n:
                raise ValueError("PathDeposit: within has shape %s, the grid %s" % (shp, self._n))
        if self._on_device:
            if within is not None:
                self.d_within = grid.layout.to_layout(within, torch.uint8)
            if not getattr(grid, '_device_mask', False):         # the mask was uploaded from the host: from now on it lives here
                grid.set_mask_device(grid.d_mask, all_solid=False)
            self._count = torch.zeros(1, dtype=torch.int64, device=_device())

    # ---- the definition
    @staticmethod
    def reference_terms(path, bead, shape, dx, t, dt):
        """the terms of `reference` for every piece of the step that deposits, in segment order: (k, r2, h2, z, cap), arrays that
        broadcast to `shape` -- r2 the squared distance from the piece of path travelled and h2 its bound, z the depth offset from
        the path point and cap the bead's height there.  One fp64 operation per line, in the order the library performs them."""
        p = path._path if isinstance(path, ScanPathSource) else path
        w, h = bead.validate()
        t, dt, dx = float(t), ScanPath._num(dt, 'dt', positive=True), float(dx)
        x = [(np.arange(n, dtype=np.float64) + 0.5) * dx for n in shape]
        X = (x[0][:, None, None], x[1][None, :, None], x[2][None, None, :])
        (u, v), da = p.axes, int(p.depth_axis)
        for k in range(len(p._seg)):
            _, p0, _, d, vel, _ = p._seg[k]
            pc = p._piece(k, t, t + dt)
            if pc is None or not vel > 0.0:                  # no power (a jump, an idle dwell) or no travel (a dwell)
                continue
            ta, tb, _ = pc
            ou = X[u] - p0[u]
            ov = X[v] - p0[v]
            z = X[da] - p0[da]
            xi0 = ou * d[0] + ov * d[1]
            y = ov * d[0] - ou * d[1]
            sa = vel * ta
            sb = vel * tb
            xc = np.minimum(np.maximum(xi0, sa), sb)
            e = xi0 - xc
            r2 = e * e + y * y
            half = 0.5 * w
            h2 = half * half
            cap = h * (1.0 - r2 / h2) if bead.profile == 'parabola' else np.full_like(r2, h)
            yield k, r2, h2, z, cap

    @staticmethod
    def reference(path, bead, shape, dx, t, dt, active=None, within=None):
        """THE DEFINITION of the cells born in the step [t, t + dt] on a grid of `shape` cells of edge dx (pure NumPy): the cells
        whose centre ((i+1/2)dx, (j+1/2)dx, (k+1/2)dx) lies within width/2 of the piece of path travelled (round ends, closed
        corners) and at most the bead's height below the path's depth coordinate, OR-ed over the depositing segments the step
        overlaps (power > 0 and speed > 0), inside `within` (where given) and not in `active` (where given) -> bool array"""
        shape = tuple(int(n) for n in shape)
        born = np.zeros(shape, dtype=bool)
        for _, r2, h2, z, cap in PathDeposit.reference_terms(path, bead, shape, dx, t, dt):
            born |= (r2 <= h2) & (z <= 0.0) & (-z <= cap)
        if within is not None:
            born &= np.asarray(within, dtype=bool)
        if active is not None:
            born &= ~np.asarray(active, dtype=bool)
        return born

    # ---- the library on the host
    def _path_args(self):
        return (ctypes.byref(self._c_shape), self.path._h_table.ctypes.data, self.path.K, self.path.t_end)

    def _host_within(self):
        w = self._within
        if w is None:
            return None
        if isinstance(w, torch.Tensor):
            w = w.cpu().numpy()
        return np.ascontiguousarray(np.asarray(w).astype(np.bool_, copy=False)).view(np.uint8)

    def born_host(self, t, dt):
        """the cells the step [t, t + dt] bears on the grid's mask as it is now, by the library on the CPU
        (adi_bead_deposit_host, no GPU needed) -> bool array"""
        active = np.ascontiguousarray(np.asarray(self.grid.mask, dtype=np.bool_)).view(np.uint8)
        if active.shape != self._n:
            raise ValueError("born_host: the mask has shape %s, the grid %s" % (active.shape, self._n))
        within = self._host_within()
        born = np.empty(self._n, dtype=np.uint8)
        check(lib.adi_bead_deposit_host(*self._path_args(), active.ctypes.data,
                                        None if within is None else within.ctypes.data, *self._n, float(self.grid.dx),
                                        float(t), float(dt), born.ctypes.data))
        return born.astype(np.bool_)

    def index_box(self, t, dt):
        """((i0, i1), (j0, j1), (k0, k1)): the index box that holds every cell the step [t, t + dt] can bear
        (adi_bead_index_box, on the host); None when no segment deposits in the step or none of its bead meets the grid"""
        box, dep = (ctypes.c_int * 6)(), ctypes.c_int(0)
        check(lib.adi_bead_index_box(*self._path_args(), *self._n, float(self.grid.dx), float(t), float(dt), box,
                                     ctypes.byref(dep)))
        b = tuple((box[2 * a], box[2 * a + 1]) for a in range(3))
        return None if (not dep.value or any(lo >= hi for lo, hi in b)) else b

    # ---- the device
    def deposit(self, T, t, dt, count=None):
        """the births of the step [t, t + dt] on the device (adi_bead_deposit): T (a DeviceField in the grid's layout) gets Ts on
        the newborn cells, the grid's device mask 1, in place; then grid.set_mask_device rebuilds flags and bricks on the planes
        [k_lo, k_hi) of axis 2 whose exposure can have changed -- the index box's planes and one either side when the path's
        depth axis is 2, every plane otherwise.  -> (k_lo, k_hi) for the caller's packs; None, and nothing launched, when the step
        bears nothing.  With `material_map=` the newborn cells also get `material_id` in the map's device id field.  `count`: optional int64 device tensor (1 element) that receives the number of newborn cells (0 when the
        step bears nothing)."""
        if not self._on_device:
            raise TypeError("PathDeposit.deposit: the grid is not a Grid3D on the device")
        g = self.grid
        t_ = _native_f64(g, T, strict="PathDeposit.deposit: T must be an fp64 device field in the grid's layout")
        box = self.index_box(t, dt)
        if box is None and count is None:
            return None
        d_active = g.d_mask
        tail = (*self._n, *g.layout.pd, g.dx, float(t), float(dt), self.Ts, _p(self._count if count is None else count), _stream())
        head = (*self._path_args()[:2], _p(self.path.d_table), self.path.K, self.path.t_end, _p(t_), _p(d_active),
                _p(self.d_within))
        mm = self.material_map
        if mm is None:
            check(lib.adi_bead_deposit(*head, *tail))
        else:
            check(lib.adi_bead_deposit_ids(*head, _p(mm._d_ids), self.material_id, *tail))
            mm._ids_stamped = True                         # the map's host copy of the ids is stale: mm.ids downloads
        if box is None:
            return None
        k_lo, k_hi = (max(0, box[2][0] - 1), min(g.nz, box[2][1] + 1)) if self.path.depth_axis == 2 else (0, g.nz)
        g.set_mask_device(d_active, k_lo, k_hi, all_solid=False)
        return k_lo, k_hi
