"""The coefficient packs of the Cartesian step: `Material`, `Params`, `AxisCoeffPack`, `exposed_mask` and
`precompute_coeff_packs_unified` (adi3d_numba_coeff.py:21-118), built on the device."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from .fields import Layout, DeviceField, _p, _stream, _as_state, _wrap


class Material:  # adi3d_numba_coeff.py:21-23
    def __init__(self, rho, cp, k):
        self.rho = float(rho); self.cp = float(cp); self.k = float(k)


class Params:  # adi3d_numba_coeff.py:25-27
    def __init__(self, dt, theta=0.5):
        self.dt = float(dt); self.theta = float(theta)


class AxisCoeffPack:
    """adi3d_numba_coeff.py:29-36.  Arrays live in HBM (`d_*` tensors, device layout); the reference's
    attribute names `.coeff / .dir_mask / .dir_val / .qflux` return host copies (drivers read
    `packs[2].qflux`, quick_compare_neumann_robin.py:104)."""

    def __init__(self, coeff, dir_mask, dir_val, qflux=None, _has_dir=None, _has_q=None, _layout=None):
        self.layout = _layout or Layout(*tuple(coeff.shape))
        L = self.layout
        self.d_coeff = L.to_layout(coeff, torch.float64)
        self.d_dir_mask = None if dir_mask is None else L.to_layout(dir_mask, torch.uint8)
        self.d_dir_val = None if dir_val is None else L.to_layout(dir_val, torch.float64)
        self.d_qflux = None if qflux is None else L.to_layout(qflux, torch.float64)
        if _has_dir is None:
            _has_dir = self.d_dir_mask is not None and bool(self.d_dir_mask.any().item())
        if _has_q is None:
            _has_q = self.d_qflux is not None and bool((self.d_qflux != 0).any().item())
        self.has_dir, self.has_q = bool(_has_dir), bool(_has_q)
        if self.has_dir and self.d_dir_val is None:
            self.d_dir_val = L.empty(zero=True)
        # Set by precompute_coeff_packs_unified only: coeff/qflux are non-zero just on cells exposed along the
        # pack's axis, so the sweep may skip loading them elsewhere.  Hand-built packs are read densely.
        self.sparse_ok = False
        self.face_consts = None        # (c-, c+, q-, q+) when built from per-face scalars (precompute_coeff_packs_unified)
        self._fractions = None         # (grid, axis, mask version) the byte accounting is evaluated from, on demand
        self._exposed_fraction = 1.0   # fraction of cells exposed along the axis
        self._dir_fraction = 1.0

    def _eval_fractions(self):
        if self._fractions is not None:
            grid, a, ver = self._fractions
            self._fractions = None
            if grid.mask_version != ver:       # the mask moved on before anybody asked: keep the dense figures
                return
            fl = grid.d_flags
            L = self.layout
            ncell = float(L.nx * L.ny * L.nz)
            inmask = (fl & 1) == 1
            self._exposed_fraction = float((inmask & (((fl >> (1 + 2 * a)) & 3) != 3)).sum().item()) / ncell
            self._dir_fraction = float(self.d_dir_mask.sum().item()) / ncell if self.has_dir else 0.0

    @property
    def exposed_fraction(self):
        self._eval_fractions()
        return self._exposed_fraction

    @property
    def dir_fraction(self):
        self._eval_fractions()
        return self._dir_fraction

    @property
    def variant(self):
        if self.has_dir:
            return _lib.SWEEP_GENERAL if self.has_q else _lib.SWEEP_NO_Q
        return _lib.SWEEP_NO_DIR if self.has_q else _lib.SWEEP_LEAN

    def _host(self, t, dtype):
        if t is None:
            return np.zeros(self.layout.shape, dtype=dtype)
        return t.cpu().contiguous().numpy().astype(dtype, copy=False)

    @property
    def bytes_per_cell(self):
        """HBM bytes per cell the sweep of this pack must move (its inputs + the output): the byte count of
        the roofline (SURVEY.md 8(d) variant rule)."""
        fe = self.exposed_fraction if self.sparse_ok else 1.0
        if self.sparse_ok and self.face_consts is not None:
            fe = 0.0                                      # per-face scalars: coeff / qflux are not read at all
        b = 8.0 + 1.0 + 8.0 + 8.0 * fe                    # in, flags, out, coeff
        if self.has_q:
            b += 8.0 * fe
        if self.has_dir:
            b += 1.0 + 8.0 * (self.dir_fraction if self.sparse_ok else 1.0)
        return b

    coeff = property(lambda self: self._host(self.d_coeff, np.float64))
    qflux = property(lambda self: self._host(self.d_qflux, np.float64))
    dir_mask = property(lambda self: self._host(self.d_dir_mask, np.bool_))
    dir_val = property(lambda self: self._host(self.d_dir_val, np.float64))


def exposed_mask(mask, face):
    """adi3d_numba_coeff.py:38-55; ValueError("bad face") for an unknown face."""
    if face not in FACES:
        raise ValueError("bad face")
    host = not isinstance(mask, (torch.Tensor, DeviceField))
    shape = tuple(mask.shape)
    assert len(shape) == 3
    L = Layout(*shape, sx=shape[1] * shape[2])
    d = L.to_layout(mask, torch.uint8)
    out = L.empty(torch.uint8)
    check(lib.adi_exposed_mask(_p(d), shape[0], shape[1], shape[2], 0, FACES.index(face), _p(out), _stream()))
    return out.cpu().numpy().astype(np.bool_) if host else out.to(torch.bool)


def _face_spec(spec, L, keep):
    """scalar / array / None -> (mode, scalar, device tensor or None)"""
    if spec is None:
        return (_lib.FACE_NONE, 0.0, None)
    if np.isscalar(spec):
        return (_lib.FACE_SCALAR, float(spec), None)
    t = L.to_layout(spec, torch.float64)
    keep.append(t)
    return (_lib.FACE_FIELD, 0.0, t)


def _face_constants(grid, mat, h_modes, h_scalars, q_modes, q_scalars):
    """per axis (c-, c+, q-, q+) as a ctypes array of 4 doubles, or None where a face of the axis carries a per-voxel field:
    what the sweeps take as `h_face_consts` instead of loading coeff / qflux at the exposed cells (adi_face_constants)"""
    consts = (ctypes.c_double * 12)()
    valid = (ctypes.c_int * 3)()
    check(lib.adi_face_constants(grid.dx, mat.rho, mat.cp, (ctypes.c_int * 6)(*h_modes), (ctypes.c_double * 6)(*h_scalars),
                                 (ctypes.c_int * 6)(*q_modes), (ctypes.c_double * 6)(*q_scalars), consts, valid))
    return [(ctypes.c_double * 4)(*consts[4 * a:4 * a + 4]) if valid[a] else None for a in range(3)]


def _fc_arg(grid, pack, sp):
    """the h_face_consts argument for a sweep of `pack` under the `sparse` word `sp`: only with sparse reads (fresh packs)"""
    fc = getattr(pack, 'face_consts', None)
    return fc if (fc is not None and (sp & 1)) else None


def _face_specs(L, robin_h, neumann, keep):
    """robin_h (None / scalar / per-voxel array / dict per face) and neumann (None / dict per face) -> the six _face_spec of
    each, in FACES order; the device copies of per-voxel fields are appended to `keep`"""
    h_specs, q_specs = [], []
    for f in FACES:
        if robin_h is None:
            h_specs.append((_lib.FACE_NONE, 0.0, None))
        elif isinstance(robin_h, dict):
            h_specs.append(_face_spec(robin_h.get(f, 0.0), L, keep))
        else:
            h_specs.append(_face_spec(robin_h, L, keep))
        q_specs.append(_face_spec(neumann.get(f) if neumann is not None else None, L, keep))
    if neumann is not None:
        for f in neumann:
            if f not in FACES:
                raise ValueError("bad face")   # exposed_mask(grid.mask, f) raises in the reference (:106)
    return h_specs, q_specs


def _face_spec_args(specs):
    """(modes, scalars, field pointers) of six _face_spec as the coefficient builds of the C ABI take them"""
    return ((ctypes.c_int * 6)(*[s[0] for s in specs]), (ctypes.c_double * 6)(*[s[1] for s in specs]),
            ptr_array([s[2].data_ptr() if s[2] is not None else None for s in specs]))


def _dirichlet_fields(L, dir_mask, dir_value):
    """-> (device dir_mask, device dir_val, any Dirichlet cell) of adi3d_numba_coeff.py:70-78; (None, None, False) without a mask"""
    if dir_mask is None:
        return None, None, False
    d_dm = L.to_layout(dir_mask, torch.uint8)
    has_dir = bool(d_dm.any().item())
    if dir_value is None:
        d_dv = L.empty(zero=True)                                   # :75-76
    elif np.isscalar(dir_value):
        d_dv = L.empty(zero=L.padded)
        d_dv.fill_(float(dir_value))                                # :77-78
    else:
        d_dv = L.to_layout(dir_value, torch.float64)
    return d_dm, d_dv, has_dir


def precompute_coeff_packs_unified(grid, mat, dir_mask=None, dir_value=None, neumann=None,
                                   robin_h=None, robin_Tinf=None):
    """adi3d_numba_coeff.py:57-118: one HIP pass builds the Robin coefficient and Neumann flux fields
    of the three axes on the device.  `robin_Tinf` is accepted and ignored, as in the reference (the
    ambient enters at step time)."""
    L = grid.layout
    d_mask = grid.sync_mask()
    keep = []
    h_specs, q_specs = _face_specs(L, robin_h, neumann, keep)
    coeff = [L.empty() for _ in range(3)]
    qflux = [L.empty() for _ in range(3)]
    check(lib.adi_build_coeffs(_p(d_mask), *grid.layout.pd, grid.dx, mat.rho, mat.cp,
                               *_face_spec_args(h_specs), *_face_spec_args(q_specs),
                               ptr_array([c.data_ptr() for c in coeff]), ptr_array([q.data_ptr() for q in qflux]),
                               _stream()))
    has_q = any(s[0] != _lib.FACE_NONE for s in q_specs)
    d_dm, d_dv, has_dir = _dirichlet_fields(L, dir_mask, dir_value)
    packs = tuple(AxisCoeffPack(coeff[a], d_dm, d_dv, qflux[a], _has_dir=has_dir, _has_q=has_q, _layout=L)
                  for a in range(3))
    fcs = _face_constants(grid, mat, [s[0] for s in h_specs], [s[1] for s in h_specs], [s[0] for s in q_specs],
                          [s[1] for s in q_specs])
    for a, p in enumerate(packs):
        p.mask_version = grid.mask_version
        p.sparse_ok = True
        p.face_consts = fcs[a]                           # per-face scalars: the sweeps need not load coeff / qflux
        p._fractions = (grid, a, grid.mask_version)      # exposed / Dirichlet fractions: evaluated when somebody asks
    return packs


# ---- several materials in one grid ---------------------------------------------------------------
def _triples(materials):
    """materials (Material objects or (rho, cp, k) triples) -> list of (rho, cp, k) floats"""
    out = []
    for m in materials:
        out.append((float(m.rho), float(m.cp), float(m.k)) if hasattr(m, 'rho') else tuple(float(v) for v in m))
    return out


def _nbr_in_mask(mask, axis, plus):
    """True where the cell is in the mask and so is its neighbour at +1 (plus) or -1 along `axis`"""
    nb = np.zeros_like(mask)
    lo = [slice(None)] * 3; hi = [slice(None)] * 3
    lo[axis] = slice(None, -1); hi[axis] = slice(1, None)
    if plus:
        nb[tuple(lo)] = mask[tuple(hi)]
    else:
        nb[tuple(hi)] = mask[tuple(lo)]
    return mask & nb


def _thomas_excess64(p, q, e, d):
    """rows along the last axis: (e + p + q) x_i - p x_{i-1} - q x_{i+1} = d with e >= 1, p, q >= 0, eliminated without a
    subtraction (fp64; p[..., 0] and q[..., -1] are 0 by construction)"""
    n = d.shape[-1]
    P = np.empty_like(d); dp = np.empty_like(d); x = np.empty_like(d)
    s = e[..., 0]
    P[..., 0] = s + q[..., 0]
    dp[..., 0] = d[..., 0]
    for i in range(1, n):
        w = p[..., i] / P[..., i - 1]
        ws = w * s
        s = e[..., i] + ws
        P[..., i] = s + q[..., i]
        wd = w * dp[..., i - 1]
        dp[..., i] = d[..., i] + wd
    x[..., n - 1] = dp[..., n - 1] / P[..., n - 1]
    for i in range(n - 2, -1, -1):
        qx = q[..., i] * x[..., i + 1]
        num = dp[..., i] + qx
        x[..., i] = num / P[..., i]
    return x


class _MapLoss:
    """What step.py names of matmap_extras.MapLossPacks (that module comes after the step's in the module map, as monitor.py
    does): the surface loss of a MaterialMap `.mm`, with `update(T, Tinf)` and `graph_key()`."""


class _MapPhase:
    """What step.py names of matmap_extras.MapPhaseField: the liquid fraction of a MaterialMap `.mm`, with `apply(T, d_dir_mask)`,
    `_check_fresh()`, `snapshot()`, `restore(s)` and `graph_key()`."""


class _MapSource:
    """What step.py names of matmap_extras.MapSource: a moving GoldakSource `.src` for the step of a MaterialMap `.mm`, with
    `set_block(blk, t0, dt)`, `shape_key()` and `add_r0(R0, params, blk)`."""


class _MapPathSource(_MapSource):
    """What step.py names of matmap_extras.MapPathSource: a ScanPathSource `.src` for the step of a MaterialMap `.mm`, with
    `add_r0(R0, params, t)`: plain launches only, the window of the step travels by value from the host (no device block, no
    graph)."""


class _MapTransitions:
    """What step.py names of matmap_extras.MaterialTransitions: the material changes of a MaterialMap `.mm` with its liquid
    fraction `.phase` (or None), with `apply(T, d_dir_mask)`, `_check_fresh()`, `snapshot()`, `restore(s)`, `graph_key()` and
    `after_replay()` (run() replayed a graph that holds the pass: the map's host copy of the ids is stale)."""


class MaterialMap:
    """A grid of several materials: 1 to 8 (rho, cp, k) and a uint8 id per cell.  The step under it couples a cell of material
    m to an in-mask neighbour of material n with the pair-table entry G[m][n] = (kf(m, n) dt) / (C_m dx^2), kf the harmonic
    mean of the two conductivities (k_m itself for m == n) and C_m = rho_m cp_m: include/adi_hip.h, "Several materials".
        mm = MaterialMap(grid, materials, ids, robin_h=..., neumann=..., dir_mask=..., dir_value=...)
        T = adi_step_numba_coeff(T, grid, mm.mat, params, mm.packs, Tinf, material_map=mm)
    `.mat` (= materials[0]) and `.packs` are what the step's `mat` and `packs` arguments must be.  The packs are built on the
    device from the id field (adi_matmap_build_coeffs) and read sparsely, at exposed cells; `face_consts` stays None.  An id
    off the mask is never read: it has to be valid when `rebuild()` finds the cell in the mask, so one id field serves a whole
    deposition run.  After `grid.mask` changed call `rebuild()`: the pack objects stay, their arrays are rewritten.  After a
    birth or a deposit `update(k_begin, k_end)` rewrites the planes it touched only and reads nothing back; it needs every id of
    the field, in or off the mask, to name a material (`ids_all_valid`).  A PathDeposit made with `material_map=` writes the id of
    its newborn cells into the device field; `ids` then downloads it.
    Lines of any length are served: up to 1024 rows in registers (segment kernels on all three axes), longer ones by one
    thread per line.  `packs_reference` and `step_reference` are the definition in NumPy fp64."""
    MAX_MATERIALS = _lib.MATMAP_MAX

    def __init__(self, grid, materials, ids, dir_mask=None, dir_value=None, neumann=None, robin_h=None):
        mats = _triples(materials)
        if not 1 <= len(mats) <= self.MAX_MATERIALS:
            raise ValueError("MaterialMap: %d materials (1 to %d)" % (len(mats), self.MAX_MATERIALS))
        for m in mats:
            if len(m) != 3 or not all(np.isfinite(v) and v > 0.0 for v in m):
                raise ValueError("MaterialMap: rho, cp and k must be finite and > 0, got %r" % (m,))
        self.grid = grid
        self.materials = tuple(Material(*m) for m in mats)
        self.mat = self.materials[0]
        self._bc = dict(dir_mask=dir_mask, dir_value=dir_value, neumann=neumann, robin_h=robin_h)
        self._ids = self._checked_ids(ids)
        self._ids_version = 0
        self._tables_for = None
        self.packs = None
        self._d_ids = grid.layout.to_layout(torch.from_numpy(self._ids), torch.uint8)
        self._ids_stamped = False       # a PathDeposit wrote ids on the device since the host copy was made
        self._specs = None              # the face specs with their device copies of per-voxel fields, made by the first build
        self._work = None
        self.rebuild()

    def _checked_ids(self, ids):
        """a host copy of `ids` after the checks of the constructor (nothing is launched before they pass)"""
        g = self.grid
        if isinstance(ids, (torch.Tensor, DeviceField)) or not isinstance(ids, np.ndarray):
            raise ValueError("MaterialMap: ids must be a NumPy uint8 array of the grid's shape")
        if ids.dtype != np.uint8:
            raise ValueError("MaterialMap: ids must be uint8, got %s" % ids.dtype)
        if tuple(ids.shape) != g.shape:
            raise ValueError("MaterialMap: ids have shape %s, the grid %s" % (tuple(ids.shape), g.shape))
        ids = np.array(ids, dtype=np.uint8, order='C')
        self._check_in_mask(ids)
        self.ids_all_valid = bool(ids.size == 0 or int(ids.max()) < len(self.materials))   # off the mask too: update() needs it
        return ids

    def _check_in_mask(self, ids):
        mask = np.asarray(self.grid.mask, dtype=bool)
        if mask.any() and int(ids[mask].max()) >= len(self.materials):
            raise ValueError("MaterialMap: an in-mask cell has id %d, there are %d materials"
                             % (int(ids[mask].max()), len(self.materials)))

    def _host_ids(self):
        """the host copy of the id field, downloaded first when a PathDeposit has stamped the device field since"""
        if self._ids_stamped:
            self._ids = np.array(self.grid.layout.to_host(self._d_ids), dtype=np.uint8, order='C')
            self._ids_stamped = False
        return self._ids

    ids = property(lambda self: self._host_ids().copy())

    def set_ids(self, ids):
        """replace the id field, on the host and on the device, then rebuild the packs"""
        self._ids = self._checked_ids(ids)
        self._ids_stamped = False
        self._d_ids = self.grid.layout.to_layout(torch.from_numpy(self._ids), torch.uint8)
        self._ids_version += 1
        self.rebuild()

    def _face_args(self):
        """the face specs of the constructor as the coefficient builds take them; the device copies of per-voxel robin_h / neumann
        fields are made once, by the first build, and live as long as the map (update() uploads nothing)"""
        if self._specs is None:
            keep = []
            h_specs, q_specs = _face_specs(self.grid.layout, self._bc['robin_h'], self._bc['neumann'], keep)
            self._specs = (h_specs, q_specs, keep)
        return self._specs[0], self._specs[1]

    def _mark_fresh(self):
        g = self.grid
        for a, p in enumerate(self.packs):
            p.mask_version = g.mask_version
            p.sparse_ok = True
            p.face_consts = None                          # C differs from cell to cell: no per-face constants
            p._fractions = (g, a, g.mask_version)

    def update(self, k_begin, k_end):
        """rebuild the planes [k_begin, k_end) of axis 2 (clipped to the box) from the grid's device mask and the device id
        field as they are now (adi_matmap_build_coeffs_planes) and mark the packs fresh for grid.mask_version -> packs.  One
        launch; nothing is uploaded, downloaded or synchronised -- so no id can be checked against the mask here, and every id
        of the field must name a material (ValueError otherwise: use rebuild())."""
        if not self.ids_all_valid:
            raise ValueError("MaterialMap.update: the id field holds an id that names no material (off the mask, where rebuild() "
                             "never reads it); update() reads no mask back, so every id must be below %d -- use rebuild(), or "
                             "set_ids() with a field whose ids are all valid" % len(self.materials))
        g, L = self.grid, self.grid.layout
        k0, k1 = max(0, int(k_begin)), min(L.pz, int(k_end))
        if k1 > k0:
            h_specs, q_specs = self._face_args()
            C = (ctypes.c_double * len(self.materials))(*[m.rho * m.cp for m in self.materials])
            check(lib.adi_matmap_build_coeffs_planes(_p(g.d_mask), _p(self._d_ids), *L.pd, g.dx, len(self.materials), C,
                                                     *_face_spec_args(h_specs), *_face_spec_args(q_specs),
                                                     ptr_array([p.d_coeff.data_ptr() for p in self.packs]),
                                                     ptr_array([p.d_qflux.data_ptr() for p in self.packs]), k0, k1, _stream()))
        self._mark_fresh()
        return self.packs

    def rebuild(self):
        """(re)build the packs for grid.mask as it is now, with the boundary specs of the constructor"""
        g, L, bc = self.grid, self.grid.layout, self._bc
        self._check_in_mask(self._host_ids())
        d_mask = g.sync_mask()
        h_specs, q_specs = self._face_args()
        first = self.packs is None
        coeff = [L.empty() for _ in range(3)] if first else [p.d_coeff for p in self.packs]
        qflux = [L.empty() for _ in range(3)] if first else [p.d_qflux for p in self.packs]
        C = (ctypes.c_double * len(self.materials))(*[m.rho * m.cp for m in self.materials])
        check(lib.adi_matmap_build_coeffs(_p(d_mask), _p(self._d_ids), *L.pd, g.dx, len(self.materials), C,
                                          *_face_spec_args(h_specs), *_face_spec_args(q_specs),
                                          ptr_array([c.data_ptr() for c in coeff]), ptr_array([q.data_ptr() for q in qflux]),
                                          _stream()))
        if first:
            has_q = any(s[0] != _lib.FACE_NONE for s in q_specs)
            d_dm, d_dv, has_dir = _dirichlet_fields(L, bc['dir_mask'], bc['dir_value'])
            self.packs = tuple(AxisCoeffPack(coeff[a], d_dm, d_dv, qflux[a], _has_dir=has_dir, _has_q=has_q, _layout=L)
                               for a in range(3))
            wb = 0
            for ax in range(3):
                b = ctypes.c_size_t(0)
                check(lib.adi_matmap_workspace_bytes(ax, *L.pd, ctypes.byref(b)))
                wb = max(wb, b.value)
            self._work = torch.empty(wb, dtype=torch.uint8, device=coeff[0].device) if wb else None
        self._mark_fresh()
        torch.cuda.current_stream().synchronize()          # (as ever: the build is done when rebuild returns)

    def graph_key(self):
        """what a captured launch holds of this map besides dt and theta: the id field by pointer, the table by value"""
        return (id(self), self._ids_version, self._d_ids.data_ptr(), tuple((m.rho, m.cp, m.k) for m in self.materials))

    @staticmethod
    def pair_table_of(materials, dx, dt):
        """the 8 x 8 table G[m][n] (zeros beyond the materials given), fp64, one operation per line"""
        mats = _triples(materials)
        G = np.zeros((_lib.MATMAP_MAX, _lib.MATMAP_MAX))
        dx2 = dx * dx
        for m, (rho_m, cp_m, k_m) in enumerate(mats):
            C_m = rho_m * cp_m
            den = C_m * dx2
            for n, (_, _, k_n) in enumerate(mats):
                if m == n:
                    kf = k_m
                else:
                    two_k = 2.0 * k_m
                    num = two_k * k_n
                    ksum = k_m + k_n
                    kf = num / ksum
                kfdt = kf * dt
                G[m, n] = kfdt / den
        return G

    def pair_table(self, dt):
        return self.pair_table_of(self.materials, self.grid.dx, float(dt))

    @property
    def bytes_per_cell(self):
        """HBM bytes per cell of one step by its data model, pack reads at exposed cells aside: the explicit stage moves T,
        flags, id and R0 (18); a sweep in, flags, id and out (18), and a thread-per-line sweep (lines beyond 1024 rows) also
        writes and re-reads c' and d' (+ 32)"""
        L = self.grid.layout
        per_line = [L.px > 1024, L.py > 1024, L.pz > 1024]
        return float(18 + sum(18 + (32 if t else 0) for t in per_line))

    # ---- launches -------------------------------------------------------------------------------------------------------
    def _tables(self, dt):
        if self._tables_for != dt:
            G = self.pair_table(dt)
            C = [m.rho * m.cp for m in self.materials]
            self._tabs = ((ctypes.c_double * G.size)(*G.ravel()), (ctypes.c_double * len(C))(*C))
            self._tables_for = dt
        return self._tabs

    def _explicit_into(self, t, d_S, out, params):
        G, C = self._tables(params.dt)
        g = self.grid
        check(lib.adi_matmap_explicit(_p(t), _p(d_S), _p(g.d_flags), _p(self._d_ids), *g.layout.pd, len(self.materials), G, C,
                                      params.dt, params.theta, _p(out), _stream()))

    def _sweep_into(self, axis, t_in, t_out, params, Tinf):
        G, _ = self._tables(params.dt)
        g, pack = self.grid, self.packs[axis]
        check(lib.adi_matmap_sweep(axis, pack.variant, _p(t_in), _p(g.d_flags), _p(self._d_ids), _p(pack.d_coeff),
                                   _p(pack.d_dir_mask), _p(pack.d_dir_val), _p(pack.d_qflux), *g.layout.pd, len(self.materials),
                                   G, params.dt, params.theta, float(Tinf), _p(t_out), _p(self._work),
                                   0 if self._work is None else self._work.numel(), _stream()))

    def _check_fresh(self):
        if any(p.mask_version != self.grid.mask_version for p in self.packs):
            raise ValueError("material_map: grid.mask changed since the packs were built; call rebuild()")

    def explicit_rhs(self, T, params, S=None):
        """R0 of the definition (stage entry point); S: a source field of the grid's shape, or None"""
        self._check_fresh()
        g = self.grid
        t, kind = _as_state(T, g)
        d_S = None if S is None else g.layout.to_layout(S, torch.float64)
        out = g.layout.empty()
        self._explicit_into(t, d_S, out, params)
        return _wrap(out, kind)

    def sweep_axis(self, axis, stage_in, params, Tinf=0.0):
        """one sweep of the definition from `stage_in` (stage entry point)"""
        self._check_fresh()
        t, kind = _as_state(stage_in, self.grid)
        out = self.grid.layout.empty()
        self._sweep_into(int(axis), t, out, params, Tinf)
        return _wrap(out, kind)

    # ---- the definition in NumPy fp64 -------------------------------------------------------------------------------------
    @staticmethod
    def packs_reference(mask, ids, materials, dx, dir_mask=None, dir_value=None, neumann=None, robin_h=None):
        """three packs (coeff, qflux, dir_mask, dir_val) as NumPy arrays: (h (dx dx)) / (C_id (dx dx dx)) summed over the exposed
        faces of the axis, '-' then '+'"""
        import types
        mask = np.asarray(mask, dtype=bool)
        shape = mask.shape
        for spec in (neumann, robin_h):
            if isinstance(spec, dict) and any(f not in FACES for f in spec):
                raise ValueError("bad face")
        C = np.array([rho * cp for rho, cp, _ in _triples(materials)])
        A = dx * dx
        V = dx * dx * dx
        idm = np.where(mask, ids, 0).astype(np.intp)
        Ccell = C[idm] * V
        dm = np.zeros(shape, bool) if dir_mask is None else np.array(dir_mask, dtype=bool)
        dv = np.zeros(shape) if dir_value is None else np.array(np.broadcast_to(np.asarray(dir_value, np.float64), shape))
        packs = []
        for axis in range(3):
            coeff = np.zeros(shape); qflux = np.zeros(shape)
            for plus in (0, 1):
                face = FACES[2 * axis + plus]
                exp = mask & ~_nbr_in_mask(mask, axis, bool(plus))
                if robin_h is not None:
                    hv = robin_h.get(face, 0.0) if isinstance(robin_h, dict) else robin_h
                    hA = np.asarray(hv, np.float64) * A
                    term = hA / Ccell
                    coeff = np.where(exp, coeff + term, coeff)
                if neumann is not None and neumann.get(face) is not None:
                    qA = np.asarray(neumann[face], np.float64) * A
                    term = qA / Ccell
                    qflux = np.where(exp, qflux + term, qflux)
            packs.append(types.SimpleNamespace(coeff=coeff, qflux=qflux, dir_mask=dm, dir_val=dv))
        return tuple(packs)

    @staticmethod
    def step_reference(T, mask, ids, materials, dx, dt, theta, packs, Tinf, S=None, return_stages=False):
        """one step of the definition in NumPy fp64, one operation per line; packs: three objects with .coeff, .qflux,
        .dir_mask, .dir_val (packs_reference's, or AxisCoeffPacks).  return_stages: also dict(R0, U, V, W)"""
        T = np.asarray(T, dtype=np.float64)
        mask = np.asarray(mask, dtype=bool)
        G = MaterialMap.pair_table_of(materials, dx, dt)
        C = np.array([rho * cp for rho, cp, _ in _triples(materials)])
        idm = np.where(mask, ids, 0).astype(np.intp)
        nbr = {(axis, plus): (_nbr_in_mask(mask, axis, plus), np.roll(idm, -1 if plus else 1, axis))
               for axis in range(3) for plus in (False, True)}
        acc = np.zeros(T.shape)
        for axis in range(3):
            for plus in (False, True):
                has, idn = nbr[axis, plus]
                Tn = np.roll(T, -1 if plus else 1, axis)
                diff = Tn - T
                term = G[idm, idn] * diff
                acc = np.where(has, acc + term, acc)
        om = 1.0 - theta
        inc = om * acc
        R0 = np.where(mask, T + inc, T)
        if S is not None:
            dtS = dt * np.asarray(S, dtype=np.float64)
            src = dtS / C[idm]
            R0 = np.where(mask, R0 + src, R0)
        tG = theta * G

        def sweep(axis, X, pack):
            dirc = mask & np.asarray(pack.dir_mask, dtype=bool)
            free = mask & ~dirc
            dtc = dt * np.asarray(pack.coeff)
            e = np.where(free, 1.0 + dtc, 1.0)
            dtq = dt * np.asarray(pack.qflux)
            rhs = X + dtq
            dtcT = dtc * Tinf
            rhs = rhs + dtcT
            d = np.where(free, rhs, np.where(dirc, np.asarray(pack.dir_val), X))
            (lo, idlo), (hi, idhi) = nbr[axis, False], nbr[axis, True]
            p = np.where(free & lo, tG[idm, idlo], 0.0)
            q = np.where(free & hi, tG[idm, idhi], 0.0)
            mv = lambda a: np.ascontiguousarray(np.moveaxis(a, axis, -1))
            return np.ascontiguousarray(np.moveaxis(_thomas_excess64(mv(p), mv(q), mv(e), mv(d)), -1, axis))

        U = sweep(0, R0, packs[0])
        V = sweep(1, U, packs[1])
        W = sweep(2, V, packs[2])
        if return_stages:
            return W, dict(R0=R0, U=U, V=V, W=W)
        return W
