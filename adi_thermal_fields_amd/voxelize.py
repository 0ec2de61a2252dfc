"""voxelize -- a closed triangle mesh to the solid voxel mask, on the MI355X.

Voxel (i, j, k) is solid exactly when its centre `origin + (index + 0.5) * dx` is inside the surface.  A ray runs along
one axis through every column of centres; each crossing toggles the voxels behind it; solid = an odd number of toggles
(csrc/adi_voxelize.hip: count -> scan -> one integer atomic XOR per crossing -> prefix XOR -> dense mask).  Edges and
vertices shared by triangles are counted once by construction, a centre on the surface counts as behind it (a box
[p, q] voxelises as [p, q)), and the result is the bit-for-bit value of the same arithmetic in NumPy doubles
(tests/voxelize_ref.py).  A column with an odd number of crossings is a *leak*: the surface is not closed there.

`load_voxel_from_stl_mm` has the reference's name, arguments and return tuple (waam_from_stl_v7_mm.py:218-318), so the
mask of a part comes from the package that runs it: STL -> mask -> `build_corrected_robin_fields` -> `run_layer_birth`.
`mesh` is a `TriangleMesh` or anything with `.triangles` (n, 3, 3).  No CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import check, lib
from .voxel_bc_correction import load_stl
from .voxel_morph import solidify_mask

__all__ = ['voxel_grid_for', 'voxelize_solid', 'load_voxel_from_stl_mm']


def _triangles(mesh):
    tri = mesh.triangles if hasattr(mesh, 'triangles') else mesh
    return np.ascontiguousarray(np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3))


def _dims(extent, dx):
    return tuple(max(1, int(math.ceil(float(e) / dx))) for e in extent)


def voxel_grid_for(mesh, dx, pad=0.0):
    """-> (origin (3,), shape): origin = bounds_min - pad and n = max(1, ceil((extent + 2 pad) / dx)) per axis, the
    reference's estimate_dims (waam_from_stl_v7_mm.py:237-241).  Host arithmetic, no GPU."""
    dx, pad = float(dx), float(pad)
    if not dx > 0.0:
        raise ValueError("voxel_grid_for: dx must be positive, got %r" % (dx,))
    tri = _triangles(mesh)
    if len(tri) == 0:
        raise ValueError("voxel_grid_for: the mesh has no triangles")
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    return lo - pad, _dims((hi - lo) + 2.0 * pad, dx)


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("voxelize needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device('cuda', torch.cuda.current_device())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _one_axis(tri, origin, dx, shape, axis, leaks, slot):
    """one ray axis -> dense uint8 (nx, ny, nz) device tensor; the leaking columns are added to leaks[slot]"""
    dev = tri.device
    nx, ny, nz = shape
    ntri = tri.shape[0]
    org = (ctypes.c_double * 3)(*origin)
    nwords = ctypes.c_long(0)
    check(lib.adi_voxelize_words(nx, ny, nz, axis, ctypes.byref(nwords)))
    words = torch.zeros(nwords.value, dtype=torch.int32, device=dev)
    offset = torch.zeros(ntri + 1, dtype=torch.int64, device=dev)
    check(lib.adi_voxelize_count(_p(tri), ntri, org, dx, nx, ny, nz, axis, ctypes.c_void_p(offset.data_ptr() + 8), _stream()))
    offset.cumsum_(0)                       # offset[t] = tiles before triangle t; offset[ntri] = all
    nitem = int(offset[-1].item())
    check(lib.adi_voxelize_toggle(_p(tri), _p(offset), ntri, nitem, org, dx, nx, ny, nz, axis, _p(words), _stream()))
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    check(lib.adi_voxelize_scan(_p(words), nx, ny, nz, axis, _p(mask),
                                ctypes.c_void_p(leaks.data_ptr() + 4 * slot), _stream()))
    return mask


def voxelize_solid(mesh, origin, dx, shape, axis=2, return_leaks=False, as_tensor=False):
    """The solid mask of a closed mesh on the grid (origin, dx, shape): NumPy bool (nx, ny, nz), or with `as_tensor` a
    device uint8 tensor that goes into Grid3D, solidify_mask and STLBoundaryCorrector as it is.  `axis` is the ray axis
    0, 1 or 2, or 'majority': all three and the cell-wise majority, the robust mode for meshes with small gaps.
    `return_leaks` adds the number of columns with an odd number of crossings (per axis, a 3-tuple, for 'majority');
    0 for a closed mesh.  An empty mesh gives an all-False mask."""
    dx = float(dx)
    if not dx > 0.0:
        raise ValueError("voxelize_solid: dx must be positive, got %r" % (dx,))
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError("voxelize_solid: bad grid shape %r" % (shape,))
    origin = [float(v) for v in np.asarray(origin, dtype=np.float64).reshape(3)]
    if axis != 'majority' and axis not in (0, 1, 2):
        raise ValueError("voxelize_solid: axis must be 0, 1, 2 or 'majority', got %r" % (axis,))
    tri = torch.from_numpy(_triangles(mesh)).to(_dev())
    axes = (0, 1, 2) if axis == 'majority' else (int(axis),)
    leaks = torch.zeros(3, dtype=torch.int32, device=tri.device)
    masks = [_one_axis(tri, origin, dx, shape, a, leaks, s) for s, a in enumerate(axes)]
    mask = masks[0]
    if axis == 'majority':
        check(lib.adi_voxelize_majority(_p(masks[0]), _p(masks[1]), _p(masks[2]), mask.numel(), _p(mask), _stream()))
    out = mask if as_tensor else mask.cpu().numpy().astype(np.bool_)
    if not return_leaks:
        return out
    n = [int(v) for v in leaks.cpu()]
    return out, (tuple(n) if axis == 'majority' else n[0])


def load_voxel_from_stl_mm(stl_path, dx_mm, pad_mm=0.0, voxel_method='ray', auto_dx=True, max_voxels=12_000_000,
                           solidify='auto', solid_close_iters=2):
    """waam_from_stl_v7_mm.py:218-318 -> (mask, origin_mm, dx_mm, shape, mesh), everything in the STL's millimetres.
    The grid is the mesh's bounding box grown by `pad_mm`; `auto_dx` coarsens dx by (N / max_voxels) ** (1/3) when the
    grid would hold more than `max_voxels`.  The mask is the solid one (`voxelize_solid(axis='majority')`), then
    `solidify_mask(mode=solidify)`, which leaves a solid mask as it is under 'auto'.  The reference's surface-shell
    voxelisers are not reproduced: voxel_method='subdivide' raises."""
    if voxel_method == 'subdivide':
        raise NotImplementedError("load_voxel_from_stl_mm: voxel_method='subdivide' (a surface shell) is not built; "
                                  "use 'ray', which gives the solid mask every consumer wants")
    mesh = load_stl(stl_path)
    if len(mesh) == 0:
        raise RuntimeError("%s: empty STL" % stl_path)
    dx_mm, pad = float(dx_mm), float(pad_mm)
    if not dx_mm > 0.0:
        raise ValueError("load_voxel_from_stl_mm: dx_mm must be positive, got %r" % (dx_mm,))
    origin, shape = voxel_grid_for(mesh, dx_mm, pad)
    n = shape[0] * shape[1] * shape[2]
    if auto_dx and n > max_voxels:
        dx_mm = dx_mm * (n / float(max_voxels)) ** (1.0 / 3.0)
        origin, shape = voxel_grid_for(mesh, dx_mm, pad)
    mask = voxelize_solid(mesh, origin, dx_mm, shape, axis='majority')
    if solidify in ('flood', 'close_flood', 'auto'):
        mask = solidify_mask(mask, mode=solidify, close_iters=int(solid_close_iters))
    return mask, tuple(float(v) for v in origin), dx_mm, shape, mesh
