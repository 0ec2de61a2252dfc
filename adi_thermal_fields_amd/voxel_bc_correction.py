"""voxel_bc_correction -- the reference's STL correction of voxel Robin coefficients on the MI355X.

Same names and argument meaning as the reference's voxel_bc_correction.py (`STLBoundaryCorrector`,
`build_corrected_robin_fields`), so quick_compare_robin_end_robin_corrected.py:174-207 switches by import.  The
reference loops over triangles and their sub-triangles in CPython (tens of microseconds each); here every sub-triangle
is one GPU thread: count -> scan -> bin -> stable sort -> per-voxel sums in the reference's order of addition -> fallback
(csrc/adi_stlcorr.hip).  No floating-point atomics: two runs give the same bits.

`mesh` is any object with `triangles` (n, 3, 3), `face_normals` (n, 3) and `area_faces` (n) -- a trimesh.Trimesh, or the
`TriangleMesh` below, which needs nothing but NumPy (`load_stl` reads binary and ASCII STL files into one).  A NumPy
mask gives NumPy fields; a device mask (torch tensor or DeviceField) gives device tensors in the layout of
`Grid3D(...).layout`, which `precompute_coeff_packs_unified(robin_h=...)` takes without a copy.  No CPU fallback.
"""
import ctypes
import struct

import numpy as np
import torch

from . import _lib
from ._lib import FACES, check, lib, ptr_array
from .fields import DeviceField, Layout

__all__ = ['STLBoundaryCorrector', 'build_corrected_robin_fields', 'TriangleMesh', 'load_stl']


class TriangleMesh:
    """The four per-triangle arrays the corrector reads from a trimesh.Trimesh, from the vertices alone:
    `triangles` (n, 3, 3), `triangles_center`, `face_normals` (unit; zero for a degenerate triangle) and `area_faces`.
    The normal follows the winding: (v1 - v0) x (v2 - v0)."""

    def __init__(self, triangles):
        tri = np.array(triangles, dtype=np.float64).reshape(-1, 3, 3)
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        cross = np.stack([cx, cy, cz], axis=1)
        norm = np.sqrt((cx * cx + cy * cy) + cz * cz)
        self.triangles = tri
        self.triangles_center = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.0
        self.area_faces = 0.5 * norm
        with np.errstate(invalid='ignore', divide='ignore'):
            self.face_normals = np.where(norm[:, None] > 0.0, cross / norm[:, None], 0.0)

    def __len__(self):
        return len(self.triangles)


def load_stl(path, scale=1.0):
    """Binary or ASCII STL file -> TriangleMesh, vertices multiplied by `scale` (1e-3 for a file in millimetres).
    The normals stored in the file are ignored (many writers leave them zero); they are recomputed from the winding."""
    with open(path, 'rb') as f:
        data = f.read()
    tri = None
    if len(data) >= 84:
        n = struct.unpack_from('<I', data, 80)[0]
        if len(data) == 84 + 50 * n:          # a binary file's length follows from its count; "solid" in the header proves nothing
            rec = np.frombuffer(data, dtype=np.dtype([('n', '<f4', 3), ('v', '<f4', (3, 3)), ('a', '<u2')]), count=n,
                                offset=84)
            tri = rec['v'].astype(np.float64)
    if tri is None:
        verts = []
        for line in data.decode('ascii', 'replace').splitlines():
            w = line.split()
            if len(w) == 4 and w[0].lower() == 'vertex':
                verts.append((float(w[1]), float(w[2]), float(w[3])))
        if not data.lstrip().lower().startswith(b'solid') or len(verts) % 3:
            raise ValueError("%s: neither a binary STL (84 + 50 n bytes) nor an ASCII one" % path)
        tri = np.array(verts, dtype=np.float64).reshape(-1, 3, 3)
    return TriangleMesh(tri * float(scale))


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("voxel_bc_correction needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    return torch.device('cuda', torch.cuda.current_device())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f64(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    return torch.from_numpy(a).to(_dev())


class _Slots:
    """the mesh binned into the mask: sorted voxel keys, the slot of each sorted entry, per-slot area and triangle"""
    __slots__ = ('n', 'key', 'order', 'sub_area', 'slot_tri', 'normal')


class STLBoundaryCorrector:
    """voxel_bc_correction.py:32-167.  `compute_voxel_projected_areas` (a dict of Python objects per voxel) becomes
    `projected_area_fields` (six dense fields); `build_corrected_fields` is the reference's."""

    def __init__(self, mesh, mask, origin, dx, max_subdiv=6, area_epsilon=1e-16):
        self.mesh = mesh
        self.on_device = isinstance(mask, (torch.Tensor, DeviceField))
        if self.on_device:
            t = mask.t if isinstance(mask, DeviceField) else mask
            assert t.dim() == 3, tuple(t.shape)
            self.mask = t
            self.shape = tuple(int(n) for n in t.shape)
        else:
            self.mask = np.asarray(mask, dtype=bool)
            assert self.mask.ndim == 3, self.mask.shape
            self.shape = self.mask.shape
        self.origin = np.asarray(origin, dtype=float)
        assert self.origin.shape == (3,), self.origin.shape
        self.dx = float(dx)
        self.max_subdiv = max(1, int(max_subdiv))
        self.area_epsilon = float(area_epsilon)
        if not self.dx > 0.0:
            raise ValueError("STLBoundaryCorrector: dx must be positive, got %r" % (dx,))
        if self.max_subdiv > _lib.STLCORR_MAX_SUBDIV:
            raise ValueError("STLBoundaryCorrector: max_subdiv %d above %d" % (self.max_subdiv, _lib.STLCORR_MAX_SUBDIV))

    # ---- device plumbing ------------------------------------------------------------------------------------------
    def _layout(self):
        nx, ny, nz = self.shape
        return Layout(nx, ny, nz) if self.on_device else Layout(nx, ny, nz, sx=ny * nz)

    def _device_mask(self, L):
        if self.on_device:
            t = self.mask.to(device=_dev())
            if L.is_native(t) and t.dtype == torch.uint8:
                return t
            return L.to_layout((t != 0).to(torch.uint8), torch.uint8)
        return L.to_layout(self.mask, torch.uint8)

    def _bin(self, L, d_mask):
        """count -> exclusive scan -> bin -> stable sort"""
        tri = _f64(self.mesh.triangles, (-1, 3, 3))
        ntri = tri.shape[0]
        area = _f64(self.mesh.area_faces, (ntri,))
        s = _Slots()
        s.normal = _f64(self.mesh.face_normals, (ntri, 3))
        dev = _dev()
        offset = torch.zeros(ntri + 1, dtype=torch.int64, device=dev)
        check(lib.adi_stlcorr_count(_p(tri), _p(area), ntri, self.dx, self.max_subdiv, self.area_epsilon,
                                    ctypes.c_void_p(offset.data_ptr() + 8), _stream()))
        offset.cumsum_(0)                   # offset[t] = slots before triangle t; offset[ntri] = all
        s.n = int(offset[-1].item())
        key = torch.empty(s.n, dtype=torch.int64, device=dev)
        s.sub_area = torch.empty(s.n, dtype=torch.float64, device=dev)
        s.slot_tri = torch.empty(s.n, dtype=torch.int64, device=dev)
        nx, ny, nz = self.shape
        check(lib.adi_stlcorr_bin(_p(tri), _p(area), _p(offset), ntri, s.n, _p(d_mask), nx, ny, nz, L.sx, L.pz,
                                  (ctypes.c_double * 3)(*[float(v) for v in self.origin]), self.dx, self.max_subdiv,
                                  _p(key), _p(s.sub_area), _p(s.slot_tri), _stream()))
        s.key, s.order = torch.sort(key, stable=True)         # equal keys stay in slot order
        return s

    def _accumulate(self, s, base, area, robin, scale):
        ptrs = lambda fs: ptr_array([f.data_ptr() if f is not None else None for f in fs])
        check(lib.adi_stlcorr_accumulate(_p(s.key), _p(s.order), _p(s.sub_area), _p(s.slot_tri), _p(s.normal), s.n, self.dx,
                                         (ctypes.c_double * 6)(*base), ptrs(area), ptrs(robin), ptrs(scale), _stream()))

    def _out(self, L, t):
        return t if self.on_device else L.to_host(t)

    # ---- the reference's surface ----------------------------------------------------------------------------------
    def projected_area_fields(self):
        """{face: (nx, ny, nz) field} for the six faces: the mesh area projected onto that face of each voxel, in m^2
        (the dense form of compute_voxel_projected_areas, voxel_bc_correction.py:53-110)."""
        L = self._layout()
        s = self._bin(L, self._device_mask(L))
        area = [L.empty(zero=True) for _ in FACES]
        self._accumulate(s, [0.0] * 6, area, [None] * 6, [None] * 6)
        return {f: self._out(L, a) for f, a in zip(FACES, area)}

    def build_corrected_fields(self, base_h, fallback_to_base=True):
        """voxel_bc_correction.py:112-167 -> (robin_h_fields, area_scale_fields), keyed by the faces of `base_h`."""
        L = self._layout()
        d_mask = self._device_mask(L)
        s = self._bin(L, d_mask)
        robin_f = {f: L.empty(zero=True) for f in base_h}
        scale_f = {f: L.empty(zero=True) for f in base_h}
        base = [float(base_h[f]) if f in base_h else 0.0 for f in FACES]
        live = [f in base_h and base[i] != 0.0 for i, f in enumerate(FACES)]
        self._accumulate(s, base, [None] * 6, [robin_f[f] if live[i] else None for i, f in enumerate(FACES)],
                         [scale_f[f] if live[i] else None for i, f in enumerate(FACES)])
        if fallback_to_base:
            nx, ny, nz = self.shape
            for f, v in base_h.items():
                if float(v) == 0.0:
                    continue
                if f not in FACES:
                    raise ValueError("bad face")               # exposed_mask(self.mask, face), adi3d_numba_coeff.py:54
                check(lib.adi_stlcorr_fallback(_p(d_mask), nx, ny, nz, L.sx, L.pz, FACES.index(f), float(v),
                                               _p(robin_f[f]), _p(scale_f[f]), _stream()))
        return ({f: self._out(L, t) for f, t in robin_f.items()}, {f: self._out(L, t) for f, t in scale_f.items()})


def build_corrected_robin_fields(mesh, mask, origin, dx, base_h, fallback_to_base=True, max_subdiv=6):
    """voxel_bc_correction.py:205-225"""
    corrector = STLBoundaryCorrector(mesh=mesh, mask=mask, origin=origin, dx=dx, max_subdiv=max_subdiv)
    return corrector.build_corrected_fields(base_h=base_h, fallback_to_base=fallback_to_base)
