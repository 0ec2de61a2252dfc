"""adi3d_hip_coeff -- MI355X drop-in for the reference's Cartesian ADI backends.

Same operator surface as `adi3d_numba_coeff` / `adi3d_gpu_coeff` (the reference picks a backend by
module import, waam_from_stl_v7_mm.py:321-335), so a driver switches with

    import adi_thermal_fields_amd.adi3d_hip_coeff as adi

Names and meaning follow adi3d_numba_coeff.py:14-36, :38-55, :57-118, :290-302:
    Grid3D, Material, Params, AxisCoeffPack, exposed_mask, precompute_coeff_packs_unified,
    adi_step_hip_coeff  (also exported as adi_step_numba_coeff and adi_step_gpu_coeff).

Host code is Python; every number is computed by hand-written HIP kernels reached through the
ctypes C ABI of include/adi_hip.h.  PyTorch is used only for device memory and streams.
There is no CPU fallback.

Residency: a NumPy `Tn` is uploaded, stepped and downloaded (exact reference semantics: new array
out, input untouched).  Pass a `DeviceField` (see `to_device`) to keep the state in HBM across
steps -- the step then returns a new DeviceField, like the CuPy backend returns CuPy arrays.

Device layout: fields live in HBM with a padded plane stride (`Layout.sx`, chosen by
adi_recommended_plane_stride) so that the rows of an axis-0 line do not alias on the HBM channel
interleave; the C-order (nx, ny, nz) shape of the reference is what every host-visible view has.

Mask semantics: drivers rebind `grid.mask` and then rebuild the packs
(single_track_on_plate.py:159-163, waam_from_stl_v7_mm.py:494-495, :534).  The device copy of the
mask (and its neighbour-flags digest) is refreshed on every `grid.mask = ...` assignment AND on every
precompute_coeff_packs_unified(grid, ...) call, which is the documented synchronisation point.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from ._ledger import PromiseLedger

__all__ = ['Grid3D', 'Material', 'Params', 'AxisCoeffPack', 'exposed_mask', 'precompute_coeff_packs_unified',
           'adi_step_hip_coeff', 'adi_step_numba_coeff', 'adi_step_gpu_coeff', 'DeviceField', 'to_device',
           'adi_explicit_rhs', 'adi_sweep_axis', 'StagedStepper', 'Layout', 'apply_surface_impulse_Q',
           'exposed_faces_per_layer', 'count_exposed_faces', 'perimeter_ratio', 'birth_planes', 'BirthPacks',
           'GoldakSource', 'ScanPath', 'SurfaceLoss', 'LossPacks', 'PhaseChange', 'PhaseField', 'HistoryLevels',
           'ThermalHistory']


# Mask versions come from ONE process-wide counter: a pack remembers the version of the mask it was built for, and a
# version is never shared by two grids (a per-grid counter starting at 0 let packs of grid A pass for fresh on a
# same-shape grid B and inherit A's no-fallback promise).
_MASK_VERSIONS = itertools.count(1)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("adi3d_hip_coeff needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    return torch.device('cuda', torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _sweep_workspace_bytes(nx, ny, nz, sx):
    """bytes of workspace that serve a sweep of the box along any axis (adi_sweep_workspace_bytes)"""
    wb = 0
    for ax in range(3):
        b = ctypes.c_size_t(0)
        check(lib.adi_sweep_workspace_bytes(ax, nx, ny, nz, sx, ctypes.byref(b)))
        wb = max(wb, b.value)
    return wb


def recommended_dims(nx, ny, nz):
    """physical extents the kernels want for a logical (nx, ny, nz) grid (adi_recommended_dims)"""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib.adi_recommended_dims(int(nx), int(ny), int(nz), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


class Layout:
    """Device layout of a (nx, ny, nz) grid: element (i, j, k) at i*sx + j*pz + k inside a PHYSICAL box (px, py, pz) >= the
    logical one.  Ragged extents (257 rows, nz = 250) would send every line to the GENERAL kernels, so fields are allocated
    with the extents adi_recommended_dims() picks; the cells outside the logical box are off-mask (identity rows, never
    read by an in-mask cell: the reference treats the edge of the domain and an off-mask neighbour alike,
    adi3d_numba_coeff.py:38-55), the kernels are launched on the physical box (`pd`), and everything the caller sees --
    shapes, NumPy arrays, DeviceField indexing -- is the logical box.  Layouts made with an explicit plane stride `sx`
    (slabs, views of foreign tensors) are never padded unless `phys` says so."""

    def __init__(self, nx, ny, nz, sx=None, phys=None):
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        if phys is None:
            phys = recommended_dims(nx, ny, nz) if sx is None else (self.nx, self.ny, self.nz)
        self.px, self.py, self.pz = (int(v) for v in phys)
        assert self.px >= self.nx and self.py >= self.ny and self.pz >= self.nz
        self.sx = int(lib.adi_recommended_plane_stride(self.py, self.pz)) if sx is None else int(sx)
        assert self.sx >= self.py * self.pz
        if self.px * self.sx >= _lib.MAX_BOX_CELLS:
            raise ValueError("grid %d x %d x %d: its padded box of %d x %d cells reaches the 2^32-cell limit of the "
                             "Cartesian kernels (ADI_MAX_BOX_CELLS)" % (self.nx, self.ny, self.nz, self.px, self.sx))

    @property
    def shape(self):
        return (self.nx, self.ny, self.nz)

    @property
    def strides(self):
        return (self.sx, self.pz, 1)

    @property
    def pd(self):
        """(nx, ny, nz, plane_stride) as the C ABI takes them: the physical box"""
        return (self.px, self.py, self.pz, self.sx)

    @property
    def padded(self):
        return (self.px, self.py, self.pz) != (self.nx, self.ny, self.nz)

    @property
    def numel_padded(self):
        return self.px * self.sx

    def empty(self, dtype=torch.float64, zero=False):
        buf = (torch.zeros if zero else torch.empty)(self.numel_padded, dtype=dtype, device=_device())
        return buf.as_strided(self.shape, self.strides)

    def is_native(self, t):
        return (isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == self.shape
                and tuple(t.stride()) == self.strides and t.storage_offset() == 0
                and t.untyped_storage().nbytes() >= self.numel_padded * t.element_size())

    def _fresh(self, dtype):
        # masks / flags are read over the whole physical box and the plane padding; fields over the physical box
        return self.empty(dtype, zero=(self.padded or (dtype == torch.uint8 and self.sx != self.ny * self.nz)))

    def to_layout(self, a, dtype):
        """host array / tensor / DeviceField -> tensor in this layout (a copy unless already native)."""
        if isinstance(a, DeviceField):
            a = a.t
        if isinstance(a, torch.Tensor):
            if self.is_native(a) and a.dtype == dtype:
                return a
            src = a.to(device=_device())
            if dtype == torch.uint8 and src.dtype == torch.bool:
                src = src.to(torch.uint8)
            assert tuple(src.shape) == self.shape, (tuple(src.shape), self.shape)
            out = self._fresh(dtype)
            out.copy_(src.to(dtype) if src.dtype != dtype else src)
            return out
        arr = np.asarray(a)
        if dtype == torch.uint8:
            arr = np.ascontiguousarray(arr.astype(np.bool_, copy=False)).view(np.uint8)
        else:
            arr = np.ascontiguousarray(arr, dtype=np.float64)   # fp32 fields are up-cast (waam --precision float32)
        assert tuple(arr.shape) == self.shape, (tuple(arr.shape), self.shape)
        out = self._fresh(dtype)
        es = arr.itemsize
        if self.pz == self.nz:
            # every plane of the dense host array into its (padded) device plane: ONE 2-D DMA, no staging tensor
            check(lib.adi_copy_planes(_p(out), self.sx * es, ctypes.c_void_p(arr.ctypes.data), self.ny * self.nz * es,
                                      self.ny * self.nz * es, self.nx, 1, _stream()))
        else:
            # padded rows: one dense DMA into a staging tensor, rows spread on the device
            stage = torch.empty(self.shape, dtype=dtype, device=_device())
            n = arr.size * es
            check(lib.adi_copy_planes(_p(stage), n, ctypes.c_void_p(arr.ctypes.data), n, n, 1, 1, _stream()))
            out.copy_(stage)
        torch.cuda.current_stream().synchronize()     # the caller may touch its array as soon as we return
        return out

    def to_host(self, t):
        """native-layout device tensor -> C-order NumPy array (a new array, as the reference's step returns one).  The
        array lives in page-locked memory from torch's caching host allocator: the transfer is one 2-D DMA at PCIe
        rate, and in a driver's `T = step(T, ...)` loop the block of the array dropped a step ago is reused, so no
        fresh pages are faulted in (1 GiB of first-touch page faults cost more than the transfer itself)."""
        assert self.is_native(t)
        host = torch.empty(self.shape, dtype=t.dtype, pin_memory=True)
        es = t.element_size()
        if self.pz == self.nz:
            check(lib.adi_copy_planes(ctypes.c_void_p(host.data_ptr()), self.ny * self.nz * es, _p(t), self.sx * es,
                                      self.ny * self.nz * es, self.nx, 0, _stream()))
        else:
            stage = t.contiguous()                    # padded rows: gathered on the device, one dense DMA
            n = stage.numel() * es
            check(lib.adi_copy_planes(ctypes.c_void_p(host.data_ptr()), n, _p(stage), n, n, 1, 0, _stream()))
        torch.cuda.current_stream().synchronize()
        return host.numpy()

    @staticmethod
    def of(t):
        """the layout a 3-D device tensor is in, or None when it is not of this family (rows contiguous, offset 0)"""
        if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.storage_offset() == 0 and t.stride(2) == 1
                and t.stride(1) >= t.shape[2] and t.stride(0) >= t.stride(1) * t.shape[1]):
            return None
        nx, ny, nz = t.shape
        sx, pz = t.stride(0), t.stride(1)
        py = max(ny, min(sx // pz, recommended_dims(nx, ny, nz)[1])) if pz else ny
        px = max(nx, t.untyped_storage().nbytes() // t.element_size() // sx) if sx else nx
        return Layout(nx, ny, nz, sx=sx, phys=(px, py, pz))


class DeviceField:
    """A fp64 (nx, ny, nz) field resident in HBM.  Enough of the ndarray surface for the reference's
    drivers: indexing returns NumPy data, item assignment writes through, `np.asarray(f)` downloads."""

    def __init__(self, tensor):
        assert tensor.dtype == torch.float64 and tensor.is_cuda and tensor.dim() == 3
        self.t = tensor

    shape = property(lambda self: tuple(self.t.shape))
    ndim = property(lambda self: self.t.dim())
    size = property(lambda self: self.t.numel())
    dtype = np.dtype(np.float64)

    def get(self):
        L = Layout.of(self.t)
        if L is not None and L.is_native(self.t):
            return L.to_host(self.t)
        return self.t.cpu().contiguous().numpy()

    def __array__(self, dtype=None, copy=None):
        a = self.get()
        return a if dtype is None else a.astype(dtype, copy=False)

    def copy(self):
        if self.t.is_contiguous() or self.t.storage_offset() != 0:
            return DeviceField(self.t.clone())
        # the whole storage: plane padding and the cells of the physical box outside the logical one travel along
        n = self.t.untyped_storage().nbytes() // self.t.element_size()
        flat = torch.empty(n, dtype=self.t.dtype, device=self.t.device)
        flat.copy_(self.t.as_strided((n,), (1,)))
        return DeviceField(flat.as_strided(self.t.shape, self.t.stride()))

    def astype(self, dtype, copy=True):
        return self.get().astype(dtype, copy=False)

    @staticmethod
    def _idx(idx):
        def conv(i):
            if isinstance(i, np.ndarray):
                return torch.from_numpy(np.ascontiguousarray(i)).to(_device())
            return i
        return tuple(conv(i) for i in idx) if isinstance(idx, tuple) else conv(idx)

    def __getitem__(self, idx):
        r = self.t[self._idx(idx)]
        return r.item() if r.dim() == 0 else r.cpu().numpy()

    def __setitem__(self, idx, value):
        # T[newborn] = Ts / T[idx] = Ts (waam_from_stl_v7_mm.py:489-493) and general slices
        if isinstance(value, np.ndarray):
            value = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(_device())
        elif isinstance(value, DeviceField):
            value = value.t
        self.t[self._idx(idx)] = value

    def fill_where(self, d_sel_native, value):
        """T[sel] = value with `sel` a uint8 tensor in the same device layout (HIP kernel, no host round trip)."""
        assert tuple(d_sel_native.stride()) == tuple(self.t.stride())
        n = self.t.shape[0] * self.t.stride(0)
        check(lib.adi_masked_fill(_p(self.t), _p(d_sel_native), n, float(value), _stream()))

    def min(self):
        return self.t.min().item()

    def max(self):
        return self.t.max().item()

    def sum(self):
        return self.t.sum().item()

    def mean(self):
        return self.t.mean().item()


def to_device(T):
    """NumPy (nx, ny, nz) field -> DeviceField in the library's device layout (a copy)."""
    if isinstance(T, DeviceField):
        return T.copy()
    t = Layout(*tuple(T.shape)).to_layout(T, torch.float64)
    return DeviceField(t).copy() if (isinstance(T, torch.Tensor) and t is T) else DeviceField(t)


class Grid3D:
    """adi3d_numba_coeff.py:14-19.  `mask` is a property: assigning uploads it."""

    def __init__(self, nx, ny, nz, dx, mask):
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.dx = float(dx)
        self.layout = Layout(self.nx, self.ny, self.nz)
        self._mask = None
        self._d_mask = None
        self._d_flags = None
        self._d_bricks = None
        self._all_solid = None
        self._scratch = None
        self.mask_version = next(_MASK_VERSIONS)
        if isinstance(mask, (torch.Tensor, DeviceField)):          # e.g. voxelize_solid(as_tensor=True): the setter downloads it
            self.mask = mask
        else:
            self.mask = np.asarray(mask).astype(np.bool_, copy=True, order='C')

    @property
    def shape(self):
        return (self.nx, self.ny, self.nz)

    @property
    def sx(self):
        return self.layout.sx

    @property
    def mask(self):
        if self._mask is None and self._d_mask is not None:       # device-side mask (set_mask_device): download on demand
            self._mask = self._d_mask.cpu().contiguous().numpy().astype(np.bool_)
        return self._mask

    @mask.setter
    def mask(self, m):
        if isinstance(m, (torch.Tensor, DeviceField)):
            m = np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m.get()).astype(np.bool_)
        m = np.asarray(m)
        assert m.shape == (self.nx, self.ny, self.nz)   # adi3d_numba_coeff.py:19
        self._mask = m                                   # rebinding keeps the caller's object, as in the reference
        self.sync_mask()

    def _rebuild_flags(self, k_begin=0, k_end=None):
        """neighbour flags of the device mask, in place (the buffer is zero-filled once: plane padding)"""
        if self._d_flags is None:
            self._d_flags = self.layout.empty(torch.uint8, zero=True)
        k_end = self.layout.pz if k_end is None else k_end
        check(lib.adi_build_nbr_flags_planes(_p(self._d_mask), *self.layout.pd, _p(self._d_flags),
                                             int(k_begin), int(k_end), _stream()))
        # ... and its summary over the same planes (adi_build_flag_bricks): the FAST kernels skip the flags of set bricks
        if self._d_bricks is None:
            self._d_bricks = torch.zeros(int(lib.adi_flag_bricks_words(*self.layout.pd[:3])), dtype=torch.int32,
                                         device=_device())
        check(lib.adi_build_flag_bricks(_p(self._d_flags), *self.layout.pd, _p(self._d_bricks), int(k_begin), int(k_end),
                                        _stream()))
        self.mask_version = next(_MASK_VERSIONS)
        self._all_solid = None

    @property
    def all_solid(self):
        """hint for the kernels (no surface inside the box); evaluated on demand -- it costs a host synchronisation"""
        if self._all_solid is None:
            self._all_solid = (not self.layout.padded and bool((self._d_mask != 0).all().item())) \
                if self._d_mask is not None else False       # (a padded box has off-mask cells: never "all solid")
        return self._all_solid

    @all_solid.setter
    def all_solid(self, v):
        self._all_solid = None if v is None else (bool(v) and not self.layout.padded)

    def set_mask_device(self, d_mask, k_begin=0, k_end=None, all_solid=None):
        """`grid.mask = ...` for a mask that already lives on the device (uint8 tensor in the grid's layout, e.g.
        updated in place by a birth): no host round trip; the neighbour flags are rebuilt from it (only the planes
        [k_begin, k_end) of axis 2 when the caller knows nothing else changed) and the host copy is downloaded only if
        somebody reads `grid.mask`.  `all_solid`: the caller's knowledge of the box hint (None: evaluated on demand).
        The device loop of waam.run_layer_birth uses this."""
        assert self.layout.is_native(d_mask) and d_mask.dtype == torch.uint8
        self._d_mask = d_mask
        self._mask = None
        self._device_mask = True
        self._rebuild_flags(k_begin, k_end)
        self._all_solid = None if all_solid is None else (bool(all_solid) and not self.layout.padded)
        return self._d_mask

    def sync_mask(self):
        """(Re)upload the host mask and rebuild its neighbour-flags digest; called on assignment and by
        precompute_coeff_packs_unified.  A device-side mask (set_mask_device) is authoritative as it is."""
        if getattr(self, '_device_mask', False) and self._mask is None:
            return self._d_mask
        self._device_mask = False
        new = self.layout.to_layout(self._mask, torch.uint8)
        if self._d_mask is not None and self._d_flags is not None and tuple(new.shape) == tuple(self._d_mask.shape) \
                and torch.equal(new, self._d_mask):
            # the same mask again (a second precompute_coeff_packs_unified on an unchanged grid: Dirichlet-vs-Robin
            # comparisons, packs rebuilt with another h): flags and version stand, packs built earlier stay fresh
            return self._d_mask
        self._d_mask = new
        self._rebuild_flags()
        self._all_solid = bool(np.asarray(self._mask).all()) and not self.layout.padded   # hint for the kernels: no surface inside the (physical) box
        return self._d_mask

    @property
    def d_mask(self):
        return self._d_mask

    @property
    def d_flags(self):
        """neighbour-flags digest of the mask (adi_build_nbr_flags), what the step kernels read"""
        return self._d_flags

    @property
    def d_bricks(self):
        """summary of d_flags, one bit per 16^3 brick (adi_build_flag_bricks), rebuilt with the flags; None: none kept"""
        return getattr(self, '_d_bricks', None)

    def scratch(self, n):
        """n cached scratch fields + the long-line workspace (None when not needed)."""
        if self._scratch is None or len(self._scratch[0]) < n or self._scratch[0][0].device != _device():
            # The scratch fields sit 2 KiB / 4 KiB past a 2 MiB boundary, not on it: a sweep whose input and output are both
            # 2 MiB-aligned (what separate allocations give) runs into the same channels with its reads and its writes.  Same
            # stepper, scratch as allocated against skewed, alternated (scripts/skew_probe.py, profiles/r04_q_skew_probe.txt):
            # axis-1 sweep 0.418 -> 0.409 ms, and the fused kernel's launch-to-launch spread 0.0077 -> 0.0009 ms.
            L = self.layout
            fields = []
            for i in range(n):
                skew = 256 * (i + 1)
                raw = torch.empty(L.numel_padded + skew, dtype=torch.float64, device=_device())
                fields.append(raw[skew:skew + L.numel_padded].as_strided(L.shape, L.strides))
            wb = _sweep_workspace_bytes(*L.pd)
            work = torch.empty(wb, dtype=torch.uint8, device=_device()) if wb else None
            self._scratch = (fields, work, wb)
        return self._scratch


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


def precompute_coeff_packs_unified(grid, mat, dir_mask=None, dir_value=None, neumann=None,
                                   robin_h=None, robin_Tinf=None):
    """adi3d_numba_coeff.py:57-118: one HIP pass builds the Robin coefficient and Neumann flux fields
    of the three axes on the device.  `robin_Tinf` is accepted and ignored, as in the reference (the
    ambient enters at step time)."""
    L = grid.layout
    d_mask = grid.sync_mask()
    keep = []
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

    coeff = [L.empty() for _ in range(3)]
    qflux = [L.empty() for _ in range(3)]
    hm = (ctypes.c_int * 6)(*[s[0] for s in h_specs])
    hs = (ctypes.c_double * 6)(*[s[1] for s in h_specs])
    hf = ptr_array([s[2].data_ptr() if s[2] is not None else None for s in h_specs])
    qm = (ctypes.c_int * 6)(*[s[0] for s in q_specs])
    qs = (ctypes.c_double * 6)(*[s[1] for s in q_specs])
    qf = ptr_array([s[2].data_ptr() if s[2] is not None else None for s in q_specs])
    check(lib.adi_build_coeffs(_p(d_mask), *grid.layout.pd, grid.dx, mat.rho, mat.cp,
                               hm, hs, hf, qm, qs, qf,
                               ptr_array([c.data_ptr() for c in coeff]), ptr_array([q.data_ptr() for q in qflux]),
                               _stream()))
    has_q = any(s[0] != _lib.FACE_NONE for s in q_specs)
    d_dm = d_dv = None
    has_dir = False
    if dir_mask is not None:
        d_dm = L.to_layout(dir_mask, torch.uint8)
        has_dir = bool(d_dm.any().item())
        if dir_value is None:
            d_dv = L.empty(zero=True)                                   # :75-76
        elif np.isscalar(dir_value):
            d_dv = L.empty(zero=L.padded)
            d_dv.fill_(float(dir_value))                                # :77-78
        else:
            d_dv = L.to_layout(dir_value, torch.float64)
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


def _gam(grid, mat, params):
    kappa = mat.k / (mat.rho * mat.cp)                    # adi3d_numba_coeff.py:292
    return kappa, kappa * params.dt / (grid.dx * grid.dx)


def _as_state(Tn, grid):
    """-> (device tensor in the grid's layout, kind) with kind in {'numpy', 'field', 'torch'}"""
    kind = 'field' if isinstance(Tn, DeviceField) else ('torch' if isinstance(Tn, torch.Tensor) else 'numpy')
    if kind == 'numpy':
        Tn = np.asarray(Tn)
        # Called exactly like the reference (host arrays in, host array out) the step also READS grid.mask like the
        # reference does (adi3d_numba_coeff.py:294-301 pass grid.mask to every stage): the host mask is re-uploaded and
        # compared with the device copy, so a mask mutated in place since the last assignment / pack build is seen
        # (1 B/cell next to the 16 B/cell this path moves anyway; an unchanged mask keeps flags, version and packs).
        # Device-resident stepping (DeviceField / tensor state) is the opt-in fast path: there `grid.mask = ...`,
        # grid.sync_mask() or a pack rebuild is the synchronisation point.
        if getattr(grid, '_mask', None) is not None and hasattr(grid, 'sync_mask'):
            grid.sync_mask()
    assert tuple(Tn.shape) == grid.shape
    return grid.layout.to_layout(Tn, torch.float64), kind


def _wrap(t, kind):
    if kind == 'field':
        return DeviceField(t)
    if kind == 'torch':
        return t
    return DeviceField(t).get()


def _native_f64(grid, T, strict=None):
    """T (DeviceField / tensor / array) as an fp64 device tensor in the grid's layout: itself when it is one; otherwise a
    ValueError with the text `strict`, or without `strict` a converted copy"""
    t = T.t if isinstance(T, DeviceField) else T
    if not grid.layout.is_native(t) or t.dtype != torch.float64:
        if strict is not None:
            raise ValueError(strict)
        t = grid.layout.to_layout(T, torch.float64)
    return t


def adi_explicit_rhs(Tn, grid, mat, params):
    """R0 of adi3d_numba_coeff.py:292-298 (stage entry point for per-stage parity tests / benchmarks)."""
    t, kind = _as_state(Tn, grid)
    kappa, _ = _gam(grid, mat, params)
    out = grid.layout.empty()
    check(lib.adi_explicit_rhs(_p(t), _p(grid.d_flags), *grid.layout.pd, grid.dx, params.dt,
                               kappa, params.theta, _p(out), _stream()))
    return _wrap(out, kind)


def _sparse_arg(grid, pack, dense):
    """the `sparse` argument of the sweep entry points: bit 0 = the pack arrays may be read only where the flags say a
    cell is exposed, bit 1 = all-solid box hint.  Bit 0 needs packs built for the mask the flags describe: after
    `grid.mask = new` WITHOUT a pack rebuild the reference pairs the stale packs with the live mask
    (adi3d_numba_coeff.py:150-162 reads coeff at every in-mask cell), so stale packs are read densely here too."""
    fresh = getattr(pack, 'mask_version', None) == grid.mask_version
    return int(pack.sparse_ok and fresh and not dense) | (2 if getattr(grid, 'all_solid', False) else 0)


def _ledger_key(grid, pack, entry, axis, v, sp, work, tg, plain=True):
    """-> (the PromiseLedger kept on the PACK: every stepper on it shares it; this call's key, None when not eligible)"""
    nf = pack.__dict__.get('_nofb')
    if nf is None:
        nf = pack._nofb = PromiseLedger()
    if not nf.eligible(sp, work, tg, plain):
        return nf, None
    return nf, (entry, axis, v, sp, grid.mask_version, getattr(pack, 'mask_version', None), grid.shape, grid.sx,
                None if pack.d_dir_mask is None else pack.d_dir_mask.data_ptr())


def _sweep_into(axis, t_in, t_out, grid, mat, params, pack, Tinf, variant=None, xlo=None, xhi=None, dense=False):
    _, gam = _gam(grid, mat, params)
    _, work, wb = grid.scratch(2)
    v = pack.variant if variant is None else variant
    sp = _sparse_arg(grid, pack, dense)
    nf, key = _ledger_key(grid, pack, 'sweep', axis, v, sp, work, params.theta * gam,
                          plain=not (axis == 2 and (xlo is not None or xhi is not None)))
    check(lib.adi_sweep_bricks(axis, v, _p(t_in), _p(grid.d_flags), _p(grid.d_bricks), _p(pack.d_coeff), _p(pack.d_dir_mask),
                        _p(pack.d_dir_val), _p(pack.d_qflux), *grid.layout.pd,
                        sp | nf.bit(key), params.theta,
                        gam, params.dt, float(Tinf), _p(t_out),
                        _p(xlo), _p(xhi), _fc_arg(grid, pack, sp),
                        _p(work), wb, _stream()))
    nf.learn(key, work, grid.mask_version)


def fused_supported(grid, cond_pass=False):
    """explicit stage folded into the axis-0 sweep (adi_explicit_sweep0, ABI v7) available for this grid"""
    return bool(lib.adi_explicit_fused_supported(*grid.layout.pd, 1 if cond_pass else 0))


def valid_range(t):
    """element offsets relative to t's first element that lie inside its storage: the [valid_lo, valid_hi) of
    adi_explicit_sweep0 / adi_explicit_condense0"""
    off = t.storage_offset()
    return -off, t.untyped_storage().nbytes() // t.element_size() - off


def _explicit_sweep0_into(t, t_out, grid, mat, params, pack, Tinf, variant=None, dense=False):
    """stages 1+2 of adi_step_numba_coeff (adi3d_numba_coeff.py:292-299) in one pass: R0 is evaluated inside the
    loads of the axis-0 sweep.  Neighbours are read anywhere inside t's storage."""
    kappa, gam = _gam(grid, mat, params)
    _, work, wb = grid.scratch(2)
    v = pack.variant if variant is None else variant
    vlo, vhi = valid_range(t)
    sp = _sparse_arg(grid, pack, dense)
    nf, key = _ledger_key(grid, pack, 'fused', 0, v, sp, work, params.theta * gam)
    check(lib.adi_explicit_sweep0_bricks(v, _p(t), vlo, vhi, _p(grid.d_flags), _p(grid.d_bricks), _p(pack.d_coeff),
                                         _p(pack.d_dir_mask),
                                  _p(pack.d_dir_val), _p(pack.d_qflux), *grid.layout.pd,
                                  sp | nf.bit(key), grid.dx, params.dt, kappa, params.theta,
                                  float(Tinf), _p(t_out), None, None, _fc_arg(grid, pack, sp), _p(work), wb, _stream()))
    nf.learn(key, work, grid.mask_version)


def adi_explicit_sweep_axis0(Tn, grid, mat, params, pack, Tinf=0.0, variant=None, dense=False):
    """U of adi3d_numba_coeff.py:299 straight from Tn (stage entry point of the fused kernel)."""
    t, kind = _as_state(Tn, grid)
    if variant == _lib.SWEEP_GENERAL or (variant is None and pack.variant == _lib.SWEEP_GENERAL):
        _ensure_general(pack)
    out = grid.layout.empty()
    _explicit_sweep0_into(t, out, grid, mat, params, pack, Tinf, variant, dense)
    return _wrap(out, kind)


def adi_sweep_axis(axis, stage_in, grid, mat, params, pack, Tinf=0.0, variant=None, dense=False):
    """sweep_axis0/1/2 of adi3d_numba_coeff.py:133-237 for one axis (stage entry point).
    variant=None picks the leanest kernel the pack allows; variant=_lib.SWEEP_GENERAL with dense=True forces
    the 42 B/cell general-pack kernel that reads every pack array in full, like the reference does."""
    t, kind = _as_state(stage_in, grid)
    if variant == _lib.SWEEP_GENERAL or (variant is None and pack.variant == _lib.SWEEP_GENERAL):
        _ensure_general(pack)
    out = grid.layout.empty()
    _sweep_into(axis, t, out, grid, mat, params, pack, Tinf, variant, dense=dense)
    return _wrap(out, kind)


def _ensure_general(pack):
    """materialise the arrays a forced general-pack sweep reads (zeros, like the reference's packs)"""
    L = pack.layout
    if pack.d_dir_mask is None:
        pack.d_dir_mask = L.empty(torch.uint8, zero=True)
    if pack.d_dir_val is None:
        pack.d_dir_val = L.empty(zero=True)
    if pack.d_qflux is None:
        pack.d_qflux = L.empty(zero=True)


def _check_extras(grid, mat, packs, source, surface_loss, phase, history):
    """TypeError / ValueError for an optional argument of the step that is of the wrong kind or was made for other packs, another
    grid or another cp: once per adi_step_hip_coeff call and once per StagedStepper, before anything is launched"""
    if source is not None and not isinstance(source, GoldakSource):
        raise TypeError("source must be a GoldakSource (pass a source field, e.g. ScanPath.sample_step, to "
                        "adi_step_numba_coeff)")
    if surface_loss is not None:
        if not isinstance(surface_loss, LossPacks):
            raise TypeError("surface_loss must be a LossPacks")
        if len(packs) != 3 or any(p is not q for p, q in zip(packs, surface_loss.packs)):
            raise ValueError("surface_loss: the step must be given the LossPacks' own packs (surface_loss.packs)")
    if phase is not None:
        if not isinstance(phase, PhaseField):
            raise TypeError("phase must be a PhaseField")
        if phase.grid is not grid:
            raise ValueError("phase: the PhaseField belongs to another grid")
        if float(phase.mat.cp) != float(mat.cp):
            raise ValueError("phase: the PhaseField was made for cp = %r, the step runs with %r" % (phase.mat.cp, mat.cp))
    if history is not None:
        if not isinstance(history, ThermalHistory):
            raise TypeError("history must be a ThermalHistory")
        if history.grid is not grid:
            raise ValueError("history: the ThermalHistory belongs to another grid")


def _no_mark():
    pass


def _launch_step(t_in, out, grid, mat, params, packs, Tinf, fused, d_S=None, source=None, owner=None, t_set=None,
                 surface_loss=None, phase=None, history=None, captured=False, mark=_no_mark):
    """THE launch sequence of one step t_in -> out (fp64 tensors in the grid's layout; nothing is allocated): the surface-loss
    update from t_in, the explicit stage and sweep 0 (one launch when `fused`), the moving source's correction of sweep 0's
    output, sweeps 1 and 2, the latent-heat correction of `out`, the history record.  Every form of the step calls it --
    adi_step_hip_coeff with or without a source field, StagedStepper.step, and what StagedStepper.run captures -- with
    arguments that _check_extras has passed.
    d_S: a source FIELD in the grid's layout; the explicit stage takes it (adi_explicit_rhs_src), never fused.
    source, owner: a GoldakSource and the object that holds its device block and workspace; t_set: the step's start time if the
    block is to be set here, just ahead of the correction (None: the caller has set it).
    captured: a graph may replay these launches and the caller keeps the clocks: the source's block is ticked after the
    correction, and the history launches its record without moving its host clock.  Otherwise no tick, and history.record.
    mark: called at the stage boundaries of per-stage timing: before the explicit stage, between it and sweep 0 when they are
    two launches, after sweep 0 with the source's correction, after sweep 1 and after sweep 2."""
    (ta, tb), _, _ = grid.scratch(2)
    if surface_loss is not None:
        surface_loss.update(t_in, Tinf)
    mark()
    if fused and d_S is None:
        _explicit_sweep0_into(t_in, tb, grid, mat, params, packs[0], Tinf)
    else:
        if d_S is None:
            kappa, _ = _gam(grid, mat, params)
            check(lib.adi_explicit_rhs(_p(t_in), _p(grid.d_flags), *grid.layout.pd, grid.dx, params.dt,
                                       kappa, params.theta, _p(ta), _stream()))
        else:
            _explicit_src_into(t_in, d_S, ta, grid, mat, params)
        mark()
        _sweep_into(0, ta, tb, grid, mat, params, packs[0], Tinf)
    if source is not None:
        if t_set is not None:
            source.set_block(_source_block(owner), t_set, params.dt)
        _source_lines0_into(tb, grid, mat, params, packs[0], source, owner)
        if captured:
            check(lib.adi_source_tick(_p(_source_block(owner)), _stream()))
    mark()
    _sweep_into(1, tb, ta, grid, mat, params, packs[1], Tinf)
    mark()
    _sweep_into(2, ta, out, grid, mat, params, packs[2], Tinf)
    mark()
    if phase is not None:
        phase.apply(out, packs[2].d_dir_mask if packs[2].has_dir else None)
    if history is not None:
        if captured:
            history._launch_record(t_in, out)
        else:
            history.record(t_in, out, params.dt)


def adi_step_hip_coeff(Tn, grid, mat, params, packs, Tinf=0.0, S=None, t=0.0, surface_loss=None, phase=None, history=None):
    """adi3d_numba_coeff.py:290-302 / adi3d_gpu_coeff.py:213-230: explicit stage, then the three
    implicit sweeps in the order axis 0, 1, 2.  Returns a NEW array of the kind it was given;
    `Tn` is never modified.

    S: volumetric heat source in W/m^3 (include/adi_hip.h, "Volumetric heat source"): R0 gains dt*q/(rho cp) on in-mask
    cells, q evaluated at the step's mid-time.  None: the step of the reference, the same launches as without the keyword.
    An array of the grid's shape (NumPy / torch / DeviceField): the field form -- explicit stage with the source
    (adi_explicit_rhs_src), then the three unfused sweeps.  A GoldakSource: evaluated at t + dt/2 on the device and added
    to the output of sweep 0 by superposition (adi_source_lines0), after whichever sweep-0 form the step uses.  A ScanPath is
    not accepted here: pass the field ScanPath.sample_step(grid, t, dt).
    t: the step's start time, used only by a source object.
    surface_loss: a LossPacks whose `.packs` are `packs`: their Robin coefficients are first rewritten from Tn (the law at the
    temperature at the start of the step, adi_surface_loss_update), then the step runs as above.  None: no such launch.
    phase: a PhaseField of the grid: after sweep 2 the step's output is corrected for the latent heat from the liquid fraction
    the PhaseField holds, which moves on with it (adi_phase_apply, the last launch, on the freshly allocated output).  None: no
    such launch.
    history: a ThermalHistory of the grid: the step Tn -> result (after the correction of `phase`) is recorded at the recorder's
    own clock, which moves on by dt (adi_history_record and adi_history_tick, the last launches).  None: no such launch.
    Every optional argument is checked before the first launch (_check_extras); the launches are _launch_step's."""
    if isinstance(S, ScanPath):
        raise TypeError("adi_step_hip_coeff: a ScanPath has no device evaluator; pass its field, "
                        "S=path.sample_step(grid, t, dt)")
    source = S if isinstance(S, GoldakSource) else None
    _check_extras(grid, mat, packs, source, surface_loss, phase, history)
    if history is not None:
        history._check_mask()
    t_in, kind = _as_state(Tn, grid)
    d_S = None
    if S is not None and source is None:
        if tuple(S.shape) != grid.shape:
            raise ValueError("S has shape %s, the grid %s" % (tuple(S.shape), grid.shape))
        d_S = grid.layout.to_layout(S, torch.float64)
    out = grid.layout.empty()
    _launch_step(t_in, out, grid, mat, params, packs, Tinf, fused_supported(grid), d_S=d_S, source=source, owner=grid, t_set=t,
                 surface_loss=surface_loss, phase=phase, history=history)
    return _wrap(out, kind)


def _explicit_src_into(t, d_S, out, grid, mat, params):
    kappa, _ = _gam(grid, mat, params)
    check(lib.adi_explicit_rhs_src(_p(t), _p(d_S), _p(grid.d_flags), *grid.layout.pd, grid.dx, params.dt, kappa,
                                   params.theta, mat.rho, mat.cp, _p(out), _stream()))


def _source_block(owner):
    """the device parameter block of a moving source (ADI_SOURCE_BLOCK_BYTES), one per grid / stepper / engine"""
    blk = getattr(owner, '_src_block', None)
    if blk is None or blk.device != _device():
        blk = owner._src_block = torch.zeros(_lib.SOURCE_BLOCK_BYTES, dtype=torch.uint8, device=_device())
    return blk


def _source_work(owner, dims, dx, src):
    """workspace of adi_source_lines0 on a box of `dims` = (nx, ny, nz) (lines longer than the in-register limit only; None
    otherwise), one per grid / stepper / engine, grown when a larger support needs more"""
    b = ctypes.c_size_t(0)
    check(lib.adi_source_workspace_bytes(ctypes.byref(src.as_c()), *dims, dx, ctypes.byref(b)))
    if b.value == 0:
        return None
    w = getattr(owner, '_src_work', None)
    if w is None or w.numel() < b.value or w.device != _device():
        w = owner._src_work = torch.empty(b.value, dtype=torch.uint8, device=_device())
    return w


def _source_lines0_into(U, grid, mat, params, pack, src, owner):
    """U += A0^-1 s on the axis-0 lines the support can meet (adi_source_lines0), in place; the block and the workspace
    are `owner`'s"""
    _, gam = _gam(grid, mat, params)
    sp = _sparse_arg(grid, pack, False)
    work = _source_work(owner, grid.layout.pd[:3], grid.dx, src)
    check(lib.adi_source_lines0(_p(_source_block(owner)), ctypes.byref(src.as_c()), _p(U), _p(grid.d_flags),
                                _p(pack.d_coeff), _p(pack.d_dir_mask if pack.has_dir else None), *grid.layout.pd, sp,
                                grid.dx, params.theta, gam, params.dt, mat.rho, mat.cp, _fc_arg(grid, pack, sp),
                                _p(work), 0 if work is None else work.numel(), _stream()))


class GoldakSource:
    """Goldak's double-ellipsoid heat source (Goldak, Chakravarti & Bibby 1984), axis-aligned, for the `S=` argument of
    adi_step_numba_coeff and the `source=` argument of StagedStepper.  power P [W], efficiency eta, a (transverse
    half-width), b (depth), c_f / c_r (front / rear length) [m], front fraction f_f (f_r = 2 - f_f).  The centre at time t
    is origin + travel_sign * velocity * t along travel_axis; depth_axis != travel_axis, the transverse axis is the third.
        q = 6 sqrt(3) f eta P / (a b c pi^1.5) exp(-3 xi^2/c^2 - 3 y^2/a^2 - 3 z^2/b^2),  (f, c) = (f_f, c_f) ahead of
        the centre (travel_sign*xi >= 0), (f_r, c_r) behind it; q = 0 where the exponent exceeds E_CUT = 40.
    Over all space q integrates to 2 eta P, over the half-space on one side of the centre plane normal to depth_axis to
    eta P: Goldak's normalisation for a centre on the surface.  The mask cuts the rest; nothing is renormalised.
    power, eta, f_f, origin and velocity may change between the runs of a StagedStepper without a new graph."""
    E_CUT = _lib.SOURCE_E_CUT

    def __init__(self, power, eta, a, b, c_f, c_r, f_f=0.6, origin=(0.0, 0.0, 0.0), velocity=0.0, travel_axis=1,
                 travel_sign=+1, depth_axis=2):
        self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f = power, eta, a, b, c_f, c_r, f_f
        self.origin, self.velocity = origin, velocity
        self.travel_axis, self.travel_sign, self.depth_axis = travel_axis, travel_sign, depth_axis
        self.validate()

    def validate(self):
        """ValueError for any parameter adi_heat_source rejects (include/adi_hip.h)"""
        try:
            vals = [float(v) for v in (self.power, self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f,
                                       self.velocity)]
            org = tuple(float(v) for v in self.origin)
        except (TypeError, ValueError):
            raise ValueError("GoldakSource: parameters must be real numbers, origin three of them")
        if len(org) != 3:
            raise ValueError("GoldakSource: origin must have three coordinates")
        if not all(np.isfinite(v) for v in vals + list(org)):
            raise ValueError("GoldakSource: non-finite parameter")
        P, eta, a, b, cf, cr, ff, v = vals
        if P < 0:
            raise ValueError("GoldakSource: power < 0")
        if not 0.0 <= eta <= 1.0:
            raise ValueError("GoldakSource: eta outside [0, 1]")
        if min(a, b, cf, cr) <= 0:
            raise ValueError("GoldakSource: lengths a, b, c_f, c_r must be > 0")
        if not 0.0 < ff < 2.0:
            raise ValueError("GoldakSource: f_f outside (0, 2)")
        if v < 0:
            raise ValueError("GoldakSource: velocity < 0 (the direction is travel_sign)")
        for name in ('travel_axis', 'depth_axis'):
            ax = getattr(self, name)
            if isinstance(ax, bool) or not isinstance(ax, (int, np.integer)) or not 0 <= ax <= 2:
                raise ValueError("GoldakSource: %s must be 0, 1 or 2" % name)
        if self.travel_axis == self.depth_axis:
            raise ValueError("GoldakSource: travel_axis == depth_axis")
        if self.travel_sign not in (1, -1) or isinstance(self.travel_sign, bool):
            raise ValueError("GoldakSource: travel_sign must be +1 or -1")
        return vals, org

    def as_c(self):
        (P, eta, a, b, cf, cr, ff, v), org = self.validate()
        return _lib.HeatSource(P, eta, a, b, cf, cr, ff, (ctypes.c_double * 3)(*org), v, int(self.travel_axis),
                               int(self.travel_sign), int(self.depth_axis), 0)

    def shape_key(self):
        """what the launch box of the moving-source kernel depends on (a change recaptures a stepper's graph)"""
        return (float(self.a), float(self.b), float(self.c_f), float(self.c_r), int(self.travel_axis),
                int(self.travel_sign), int(self.depth_axis))

    def center(self, t):
        c = np.array([float(v) for v in self.origin], dtype=np.float64)
        c[self.travel_axis] = c[self.travel_axis] + (float(self.travel_sign) * float(self.velocity)) * float(t)
        return c

    def q(self, x0, x1, x2, t):
        """q [W/m^3] at points (broadcast NumPy arrays, metres) -- the host evaluator, same expression as the kernels'"""
        (P, eta, a, b, cf, cr, ff, _), _ = self.validate()
        c = self.center(t)
        o = (np.asarray(x0, dtype=np.float64) - c[0], np.asarray(x1, dtype=np.float64) - c[1],
             np.asarray(x2, dtype=np.float64) - c[2])
        ta, da = self.travel_axis, self.depth_axis
        xi, y, z = o[ta], o[3 - ta - da], o[da]
        front = float(self.travel_sign) * xi >= 0.0
        f = np.where(front, ff, 2.0 - ff)
        cl = np.where(front, cf, cr)
        E = (3.0 * (xi * xi) / (cl * cl) + 3.0 * (y * y) / (a * a)) + 3.0 * (z * z) / (b * b)
        amp = (6.0 * np.sqrt(3.0) * f * eta * P) / (a * b * cl * np.pi ** 1.5)
        with np.errstate(under='ignore'):
            return np.where(E <= self.E_CUT, amp * np.exp(-np.minimum(E, 745.0)), 0.0)

    def sample(self, grid, t):
        """q at the cell centres ((i+1/2)dx, (j+1/2)dx, (k+1/2)dx) at time t: float64 array of the grid's shape, 0 off the
        mask (NumPy: the ground truth the tests hold the kernels to)"""
        dx = float(grid.dx)
        x = [(np.arange(n, dtype=np.float64) + 0.5) * dx for n in (grid.nx, grid.ny, grid.nz)]
        q = self.q(x[0][:, None, None], x[1][None, :, None], x[2][None, None, :], t)
        q = np.broadcast_to(q, (grid.nx, grid.ny, grid.nz))
        return np.where(np.asarray(grid.mask, dtype=bool), q, 0.0)

    def sample_device(self, grid, t):
        """the same on the device (adi_source_sample): a DeviceField"""
        out = grid.layout.empty()
        check(lib.adi_source_sample(ctypes.byref(self.as_c()), _p(grid.d_flags), *grid.layout.pd, grid.dx, float(t),
                                    _p(out), _stream()))
        return DeviceField(out)

    def set_block(self, blk, t0, dt, n=0):
        check(lib.adi_source_set(_p(blk), ctypes.byref(self.as_c()), float(t0), float(dt), int(n), _stream()))


_erf = np.frompyfunc(math.erf, 1, 1)


class ScanPath:
    """Goldak's double ellipsoid driven along a path of straight segments (README, "Scan paths"): the HOST definition
    of its step-averaged heat input.  A step takes it as a source field, adi_step_numba_coeff(..., S=path.sample_step(grid, t,
    dt)); a path is not accepted as `S=` itself or as `source=` of a StagedStepper (there is no device evaluator).
    Shape as GoldakSource: efficiency eta, a (half-width across the leg), b (depth), c_f / c_r (front / rear length) [m], front
    fraction f_f; depth along depth_axis, the other two axes in increasing order are the in-plane axes (u, v).  `power` [W] is
    the default of line_to.
    The path starts at `start` (metres) at time t_start; line_to adds a straight leg at constant speed (power 0: a jump with
    the beam off), dwell a stationary segment.  Segment k is active on [t_k, t_{k+1}).
    The source of a step [t, t + dt] is q_step: the exact time average of the moving source over the step, summed over the
    segments the step overlaps -- not a sample at mid-step, so a step may cross any number of legs, corners and jumps.
    The cuts bound xi and (y, z) separately: the support around the centre is a box in the leg's frame."""
    E_CUT = _lib.SOURCE_E_CUT
    DELTA_MIN = 1e-3          # travel of a piece over min(c_f, c_r) below which q_step uses Simpson's rule instead of erf

    def __init__(self, eta, a, b, c_f, c_r, f_f=0.6, depth_axis=2, power=0.0, start=(0.0, 0.0, 0.0), t_start=0.0):
        self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f = eta, a, b, c_f, c_r, f_f
        self.depth_axis, self.power = depth_axis, power
        self.validate()
        self._pos = self._point(start, 'start')
        self.start = self._pos
        self.t_start = self._num(t_start, 't_start')
        self._t_end = self.t_start
        self._seg = []            # (t_begin, p0 (3), p1 (3), (d_u, d_v), speed, power)

    @staticmethod
    def _num(v, name, positive=False, nonneg=False):
        try:
            x = float(v)
        except (TypeError, ValueError):
            raise ValueError("ScanPath: %s must be a real number" % name)
        if not np.isfinite(x):
            raise ValueError("ScanPath: non-finite %s" % name)
        if (positive and x <= 0) or (nonneg and x < 0):
            raise ValueError("ScanPath: %s must be %s" % (name, '> 0' if positive else '>= 0'))
        return x

    @classmethod
    def _point(cls, p, name):
        try:
            q = tuple(float(v) for v in p)
        except (TypeError, ValueError):
            raise ValueError("ScanPath: %s must be three real numbers" % name)
        if len(q) != 3:
            raise ValueError("ScanPath: %s must have three coordinates" % name)
        if not all(np.isfinite(v) for v in q):
            raise ValueError("ScanPath: non-finite %s" % name)
        return q

    def validate(self):
        """ValueError for a shape parameter out of range (the ranges of GoldakSource)"""
        try:
            vals = [float(v) for v in (self.eta, self.a, self.b, self.c_f, self.c_r, self.f_f, self.power)]
        except (TypeError, ValueError):
            raise ValueError("ScanPath: parameters must be real numbers")
        if not all(np.isfinite(v) for v in vals):
            raise ValueError("ScanPath: non-finite parameter")
        eta, a, b, cf, cr, ff, P = vals
        if P < 0:
            raise ValueError("ScanPath: power < 0")
        if not 0.0 <= eta <= 1.0:
            raise ValueError("ScanPath: eta outside [0, 1]")
        if min(a, b, cf, cr) <= 0:
            raise ValueError("ScanPath: lengths a, b, c_f, c_r must be > 0")
        if not 0.0 < ff < 2.0:
            raise ValueError("ScanPath: f_f outside (0, 2)")
        ax = self.depth_axis
        if isinstance(ax, bool) or not isinstance(ax, (int, np.integer)) or not 0 <= ax <= 2:
            raise ValueError("ScanPath: depth_axis must be 0, 1 or 2")
        return vals[:6]

    @property
    def axes(self):
        """(u, v): the in-plane axes"""
        da = int(self.depth_axis)
        return (1 if da == 0 else 0), (1 if da == 2 else 2)

    def _add(self, p1, d, speed, power, duration):
        self._seg.append((self._t_end, self._pos, p1, d, speed, power))
        self._pos = p1
        self._t_end = self._t_end + duration
        return self

    def line_to(self, point, speed, power=None):
        """a straight leg from the current point to `point` at `speed` [m/s]; power None: the path's default, 0: a jump.  A leg
        with power keeps the depth coordinate; a jump may move anywhere (its time is its length in space over `speed`)."""
        p1 = self._point(point, 'point')
        speed = self._num(speed, 'speed', positive=True)
        P = self._num(self.power if power is None else power, 'power', nonneg=True)
        u, v = self.axes
        du, dv, dz = p1[u] - self._pos[u], p1[v] - self._pos[v], p1[self.depth_axis] - self._pos[self.depth_axis]
        plane = math.hypot(du, dv)
        length = math.hypot(plane, dz)
        if length == 0.0:
            raise ValueError("ScanPath.line_to: a leg of zero length (use dwell)")
        if P > 0 and dz != 0.0:
            raise ValueError("ScanPath.line_to: a leg with power must keep the depth coordinate")
        duration = length / speed
        if not (np.isfinite(duration) and self._t_end + duration > self._t_end):
            raise ValueError("ScanPath.line_to: the leg takes no time at this speed")
        if plane > 0.0:
            d, vel = (du / plane, dv / plane), plane / duration if dz != 0.0 else speed
            n = math.hypot(*d)
            d = (d[0] / n, d[1] / n)
        else:
            d, vel = (1.0, 0.0), 0.0
        return self._add(p1, d, vel, P, duration)

    def dwell(self, duration, power=0.0):
        """a stationary segment; with power the ellipsoid keeps the direction of the leg before it ((1, 0) at the start)"""
        duration = self._num(duration, 'duration', positive=True)
        P = self._num(power, 'power', nonneg=True)
        if not self._t_end + duration > self._t_end:
            raise ValueError("ScanPath.dwell: the dwell takes no time")
        d = self._seg[-1][3] if self._seg else (1.0, 0.0)
        return self._add(self._pos, d, 0.0, P, duration)

    @classmethod
    def raster(cls, lo, hi, hatch, speed, power, angle_deg=0.0, bidirectional=True, jump_speed=None, depth=0.0, t_start=0.0,
               **shape):
        """a hatch over the in-plane rectangle lo = (u_lo, v_lo) .. hi = (u_hi, v_hi) at depth coordinate `depth`: parallel
        tracks along (cos, sin)(angle_deg) spaced `hatch` apart along the normal (-sin, cos), the first through the corner with
        the lowest normal coordinate, each clipped to the rectangle.  bidirectional: every other track runs backwards and a
        jump (power 0, jump_speed, default `speed`) joins the end of a track to the start of the next; otherwise every track
        runs forwards and the jump flies back."""
        ulo, vlo = (cls._num(x, 'lo') for x in lo)
        uhi, vhi = (cls._num(x, 'hi') for x in hi)
        hatch = cls._num(hatch, 'hatch', positive=True)
        depth = cls._num(depth, 'depth')
        ang = math.radians(cls._num(angle_deg, 'angle_deg'))
        if not (uhi > ulo and vhi > vlo):
            raise ValueError("ScanPath.raster: empty rectangle")
        jump_speed = speed if jump_speed is None else jump_speed
        c, s = math.cos(ang), math.sin(ang)
        if abs(c) < 1e-15:
            c = 0.0
        if abs(s) < 1e-15:
            s = 0.0
        corners = [(ulo, vlo), (uhi, vlo), (uhi, vhi), (ulo, vhi)]
        sn = [-pu * s + pv * c for pu, pv in corners]
        n_tracks = int(math.floor((max(sn) - min(sn)) / hatch + 1e-9)) + 1
        tracks = []
        for i in range(n_tracks):
            off = min(sn) + i * hatch
            # the line {off*n + l*t}: clip l to the rectangle (slab method)
            ou, ov = -off * s, off * c
            l0, l1 = -np.inf, np.inf
            ok = True
            for o, dcomp, a0, a1 in ((ou, c, ulo, uhi), (ov, s, vlo, vhi)):
                if dcomp == 0.0:
                    ok = ok and (a0 - 1e-12 * max(1.0, abs(a0)) <= o <= a1 + 1e-12 * max(1.0, abs(a1)))
                else:
                    la, lb = (a0 - o) / dcomp, (a1 - o) / dcomp
                    l0, l1 = max(l0, min(la, lb)), min(l1, max(la, lb))
            if ok and l1 - l0 > 1e-9 * hatch:
                tracks.append(((ou + l0 * c, ov + l0 * s), (ou + l1 * c, ov + l1 * s)))
        if not tracks:
            raise ValueError("ScanPath.raster: no track fits the rectangle")
        da = shape.get('depth_axis', 2)
        u, v = (1 if da == 0 else 0), (1 if da == 2 else 2)

        def pt(q):
            p = [0.0, 0.0, 0.0]
            p[u], p[v], p[da] = q[0], q[1], depth
            return tuple(p)
        path = None
        for i, (q0, q1) in enumerate(tracks):
            if bidirectional and i % 2 == 1:
                q0, q1 = q1, q0
            if path is None:
                path = cls(power=power, start=pt(q0), t_start=t_start, **shape)
            else:
                path.line_to(pt(q0), jump_speed, power=0.0)
            path.line_to(pt(q1), speed)
        return path

    # ---- plain readings
    @property
    def t_end(self):
        return self._t_end

    @property
    def n_segments(self):
        return len(self._seg)

    def _t_next(self, k):
        return self._seg[k + 1][0] if k + 1 < len(self._seg) else self._t_end

    def _index(self, t):
        """segment active at time t (a boundary belongs to the later segment); None outside [t_start, t_end)"""
        if not self._seg or t < self.t_start or t >= self._t_end:
            return None
        return int(np.searchsorted([s[0] for s in self._seg], t, side='right')) - 1

    def center(self, t):
        """the centre at time t: the start before t_start, the last point from t_end on"""
        t = float(t)
        k = self._index(t)
        if k is None:
            return np.array(self.start if (t < self.t_start or not self._seg) else self._pos, dtype=np.float64)
        tb, p0, p1 = self._seg[k][:3]
        lam = (t - tb) / (self._t_next(k) - tb)
        return np.array([a + (b - a) * lam for a, b in zip(p0, p1)], dtype=np.float64)

    def power_at(self, t):
        k = self._index(float(t))
        return 0.0 if k is None else self._seg[k][5]

    def table(self):
        """the segments as a float64 array (K, 8): t_begin, start point p[3], in-plane unit direction d[2], speed, power"""
        if not self._seg:
            raise ValueError("ScanPath: the path has no segment")
        return np.array([[tb, p0[0], p0[1], p0[2], d[0], d[1], vel, P] for tb, p0, _, d, vel, P in self._seg], dtype=np.float64)

    # ---- the definition
    def _piece(self, k, t, t1):
        """(ta, tb, w): the piece of segment k inside [t, t1] as times since its start and its length; None if it deposits
        nothing"""
        tb, _, _, _, _, P = self._seg[k]
        if not P > 0.0:
            return None
        tau0 = max(t, tb)
        tau1 = min(t1, self._t_next(k))
        if not tau1 > tau0:
            return None
        return tau0 - tb, tau1 - tb, tau1 - tau0

    def _qi(self, P, xi, Et):
        """the instantaneous double ellipsoid at along-leg offset xi, Et the exponent of the other two axes (no cut of its own)"""
        eta, a, b, cf, cr, ff = self.validate()
        front = xi >= 0.0
        f = np.where(front, ff, 2.0 - ff)
        cl = np.where(front, cf, cr)
        E = 3.0 * (xi * xi) / (cl * cl) + Et
        amp = (6.0 * np.sqrt(3.0) * f * eta * P) / (a * b * cl * np.pi ** 1.5)
        with np.errstate(under='ignore'):
            return amp * np.exp(-E)

    def _qbar(self, k, x0, x1, x2, t, dt, branch=None):
        """qbar_k at points (broadcast arrays): the time average over [t, t + dt] of the moving source during its overlap with
        segment k.  branch: None -- the definition; 'erf' / 'simpson' force one of the two forms (tests)."""
        eta, a, b, cf, cr, ff = self.validate()
        shape = np.broadcast(x0, x1, x2).shape
        out = np.zeros(shape, dtype=np.float64)
        pc = self._piece(k, t, t + dt)
        if pc is None:
            return out
        ta, tb, w = pc
        _, p0, _, d, vel, P = self._seg[k]
        u, v = self.axes
        o = (x0 - p0[0], x1 - p0[1], x2 - p0[2])
        ou, ov, z = o[u], o[v], o[self.depth_axis]
        xi0 = ou * d[0] + ov * d[1]
        y = ov * d[0] - ou * d[1]
        xia = xi0 - vel * ta
        xib = xi0 - vel * tb
        Et = 3.0 * (y * y) / (a * a) + 3.0 * (z * z) / (b * b)
        R = np.sqrt(self.E_CUT / 3.0)
        ok = np.broadcast_to((Et <= self.E_CUT) & (xib <= R * cf) & (xia >= -(R * cr)), shape)
        if not ok.any():
            return out
        xi0, xia, xib, Et = (np.broadcast_to(q, shape)[ok] for q in (xi0, xia, xib, Et))
        travel = vel * w
        delta = travel / min(cf, cr)
        if branch == 'erf' or (branch is None and delta >= self.DELTA_MIN):
            s3 = np.sqrt(3.0)
            Ff = _erf(s3 * np.maximum(xia, 0.0) / cf).astype(np.float64) - _erf(s3 * np.maximum(xib, 0.0) / cf).astype(np.float64)
            Fr = _erf(s3 * np.minimum(xia, 0.0) / cr).astype(np.float64) - _erf(s3 * np.minimum(xib, 0.0) / cr).astype(np.float64)
            brace = ff * Ff + (2.0 - ff) * Fr
            amp = (3.0 * eta * P) / (np.pi * a * b * vel * dt)
            with np.errstate(under='ignore'):
                val = (amp * np.exp(-Et)) * brace
        elif travel == 0.0:
            val = (w / dt) * self._qi(P, xia, Et)
        else:
            xim = xi0 - vel * (0.5 * (ta + tb))
            qs = (self._qi(P, xia, Et) + 4.0 * self._qi(P, xim, Et)) + self._qi(P, xib, Et)
            val = (w / dt) * (qs / 6.0)
        out[ok] = val
        return out

    def q_step(self, x0, x1, x2, t, dt):
        """the source of the step [t, t + dt] in W/m^3 at points (broadcast NumPy arrays, metres): the sum over the segments, in
        ascending order, of their time averages: one fp64 operation per line"""
        t, dt = float(t), self._num(dt, 'dt', positive=True)
        x0, x1, x2 = (np.asarray(x, dtype=np.float64) for x in (x0, x1, x2))
        q = np.zeros(np.broadcast(x0, x1, x2).shape, dtype=np.float64)
        for k in range(len(self._seg)):
            if self._piece(k, t, t + dt) is not None:
                q += self._qbar(k, x0, x1, x2, t, dt)
        return q

    def _index_box(self, k, pc, n, dx):
        """slices of the cells of an n[0] x n[1] x n[2] grid whose centres can lie in the support of piece pc of segment k: the
        support reaches R hypot(max(c_f, c_r), a) from the centre in the plane and R b in depth (the cuts of _qbar)"""
        eta, a, b, cf, cr, ff = self.validate()
        R = np.sqrt(self.E_CUT / 3.0)
        _, p0, _, d, vel, _ = self._seg[k]
        u, v = self.axes
        dirs = {u: d[0], v: d[1], int(self.depth_axis): 0.0}
        sl = []
        for ax in range(3):
            m = (R * b if ax == self.depth_axis else R * math.hypot(max(cf, cr), a)) * (1.0 + 1e-9)
            ca, cb = p0[ax] + dirs[ax] * (vel * pc[0]), p0[ax] + dirs[ax] * (vel * pc[1])
            lo = int(min(max(math.floor((min(ca, cb) - m) / dx - 0.5), 0), n[ax]))
            hi = int(min(max(math.ceil((max(ca, cb) + m) / dx - 0.5) + 1, 0), n[ax]))
            sl.append(slice(lo, max(hi, lo)))
        return tuple(sl)

    def sample_step(self, grid, t, dt):
        """q_step at the cell centres ((i+1/2)dx, (j+1/2)dx, (k+1/2)dx): float64 array of the grid's shape, 0 off the mask: the
        source field of the step, for `S=`.  Every segment is evaluated on the index box of its support only (the cells outside
        it get exactly 0 from q_step), so the temporaries are of the size of the support, not of the grid."""
        t, dt = float(t), self._num(dt, 'dt', positive=True)
        dx = float(grid.dx)
        n = (grid.nx, grid.ny, grid.nz)
        x = [(np.arange(m, dtype=np.float64) + 0.5) * dx for m in n]
        q = np.zeros(n, dtype=np.float64)
        for k in range(len(self._seg)):
            pc = self._piece(k, t, t + dt)
            if pc is None:
                continue
            si, sj, sk = self._index_box(k, pc, n, dx)
            q[si, sj, sk] += self._qbar(k, x[0][si, None, None], x[1][None, sj, None], x[2][None, None, sk], t, dt)
        return np.where(np.asarray(grid.mask, dtype=bool), q, 0.0)


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


# ---- temperature-dependent surface loss: radiation, h(T) tables (include/adi_hip.h) ------------
class SurfaceLoss:
    """Surface loss that depends on the cell's own temperature: per face a constant convection coefficient `h`, grey-body
    radiation with `emissivity` linearised about the ambient, and an optional piecewise-linear table h(T).
    h, emissivity: a scalar (every face) or a dict face -> scalar over 'x-', 'x+', 'y-', 'y+', 'z-', 'z+' (a missing face: 0,
    as for the reference's robin_h dict).  table: (T_knots, h_values), 2 to 16 strictly increasing knots in the field's unit,
    clamped to the end values outside; it is added on every face whose h or emissivity entry is non-zero.  T_offset: field
    unit -> kelvin.  The ambient of the radiation term is the step's Tinf, the one the Robin term relaxes to.
    The coefficient of a step is evaluated at the cell's temperature at the START of that step (lagged, first order in dt);
    `h_of` is the definition, adi_surface_loss_update the same operations on the device."""
    SIGMA = _lib.SURFACE_LOSS_SIGMA
    MAX_KNOTS = _lib.SURFACE_LOSS_MAX_KNOTS

    def __init__(self, h=0.0, emissivity=0.0, table=None, T_offset=273.15):
        self.h, self.emissivity, self.table, self.T_offset = h, emissivity, table, T_offset
        self.validate()

    @staticmethod
    def _per_face(spec, name):
        if isinstance(spec, dict):
            for f in spec:
                if f not in FACES:
                    raise ValueError("bad face")
            vals = [spec.get(f, 0.0) for f in FACES]
        else:
            vals = [spec] * 6
        try:
            vals = [float(v) for v in vals]
        except (TypeError, ValueError):
            raise ValueError("SurfaceLoss: %s must be a real number or a dict face -> real number" % name)
        if not all(np.isfinite(v) for v in vals):
            raise ValueError("SurfaceLoss: non-finite %s" % name)
        return vals

    def validate(self, Tinf=None):
        """ValueError for anything adi_surface_loss rejects (include/adi_hip.h); with `Tinf`, also an ambient at or below
        0 K.  -> (h[6], emissivity[6], knots, values, T_offset) as floats / float64 arrays"""
        hs = self._per_face(self.h, 'h')
        es = self._per_face(self.emissivity, 'emissivity')
        if min(hs) < 0.0:
            raise ValueError("SurfaceLoss: h < 0")
        if min(es) < 0.0 or max(es) > 1.0:
            raise ValueError("SurfaceLoss: emissivity outside [0, 1]")
        xp = fp = np.zeros(0, dtype=np.float64)
        if self.table is not None:
            try:
                xp, fp = (np.array(v, dtype=np.float64) for v in self.table)
            except (TypeError, ValueError):
                raise ValueError("SurfaceLoss: table must be (T_knots, h_values)")
            if xp.ndim != 1 or xp.shape != fp.shape or xp.size < 2:
                raise ValueError("SurfaceLoss: a table has at least 2 knots and as many values")
            if xp.size > self.MAX_KNOTS:
                raise ValueError("SurfaceLoss: more than %d knots" % self.MAX_KNOTS)
            if not (np.isfinite(xp).all() and np.isfinite(fp).all()):
                raise ValueError("SurfaceLoss: non-finite table entry")
            if not (np.diff(xp) > 0.0).all():
                raise ValueError("SurfaceLoss: knots do not increase")
        off = float(self.T_offset)
        if not np.isfinite(off):
            raise ValueError("SurfaceLoss: non-finite T_offset")
        if Tinf is not None and not float(Tinf) + off > 0.0:
            raise ValueError("SurfaceLoss: Tinf + T_offset <= 0 (the ambient in kelvin)")
        return hs, es, xp, fp, off

    def h_of(self, T, face, Tinf):
        """h [W/m^2/K] on `face` for cell temperatures T (ndarray) and ambient Tinf: THE DEFINITION of the law -- one fp64
        operation per line, in the order the kernel performs them"""
        if face not in FACES:
            raise ValueError("bad face")
        hs, es, xp, fp, off = self.validate(Tinf)
        i = FACES.index(face)
        h_face, eps = hs[i], es[i]
        T = np.asarray(T, dtype=np.float64)
        Tk = T + off
        Ta = float(Tinf) + off
        r1 = eps * self.SIGMA
        r2 = Tk * Tk
        r3 = Ta * Ta
        r4 = r2 + r3
        r5 = r1 * r4
        r6 = Tk + Ta
        rad = r5 * r6
        tab = 0.0
        if xp.size and (h_face != 0.0 or eps != 0.0):
            j = np.clip(np.searchsorted(xp, T, side='right') - 1, 0, xp.size - 2)      # xp[j] <= T < xp[j+1]
            d1 = fp[1:] - fp[:-1]
            d2 = xp[1:] - xp[:-1]
            slope = d1 / d2
            t1 = T - xp[j]
            t2 = slope[j] * t1
            tab = fp[j] + t2
            tab = np.where(T < xp[0], fp[0], tab)
            tab = np.where(T >= xp[-1], fp[-1], tab)
        h1 = h_face + tab
        return h1 + rad

    def as_c(self, Tinf=None):
        hs, es, xp, fp, off = self.validate(Tinf)
        knots = (ctypes.c_double * 16)(*xp)
        vals = (ctypes.c_double * 16)(*fp)
        return _lib.SurfaceLossLaw((ctypes.c_double * 6)(*hs), (ctypes.c_double * 6)(*es), off, int(xp.size), 0, knots, vals)

    def key(self):
        """every parameter of the law: a launch takes it by value, so a captured graph holds the law of its capture"""
        hs, es, xp, fp, off = self.validate()
        return (tuple(hs), tuple(es), tuple(xp.tolist()), tuple(fp.tolist()), off)


class LossPacks:
    """The coefficient packs of a body that loses heat by a SurfaceLoss: `.packs` are three AxisCoeffPack whose Robin
    coefficient arrays are REWRITTEN IN PLACE on the device from the temperature field (adi_surface_loss_update); the sweeps read
    them per voxel on exposed rows, as for any pack built from robin_h arrays.  Dirichlet cells and Neumann fluxes come from one
    ordinary precompute_coeff_packs_unified call here.  The d_coeff pointers never change, so a StagedStepper's graph and the
    no-fallback promise (which depends on the flags, not on coefficient values) survive every update.
        update(T)                  before a step: the exposed cells only; no allocation, no host synchronisation
        rebuild(T, k_begin, k_end) after `grid.mask` changed on those planes of axis 2 (default: the whole box): every cell,
                                   zeros where a cell is no longer exposed; Neumann fluxes of the planes rebuilt as well
    T (optional, here): the field the arrays are evaluated from at once; without it they hold zeros until the first update /
    rebuild, which the step performs itself when it is given `surface_loss=`."""

    def __init__(self, grid, mat, loss, Tinf, dir_mask=None, dir_value=None, neumann=None, T=None):
        if not isinstance(loss, SurfaceLoss):
            raise TypeError("LossPacks: loss must be a SurfaceLoss")
        loss.validate(Tinf)
        self.grid, self.mat, self.loss, self.Tinf = grid, mat, loss, float(Tinf)
        self.packs = precompute_coeff_packs_unified(grid, mat, dir_mask=dir_mask, dir_value=dir_value, neumann=neumann,
                                                    robin_h=None)
        for p in self.packs:
            p.face_consts = None                     # per-voxel coefficients: read on exposed rows (sparse_ok stays True)
        self._coeff = ptr_array([p.d_coeff.data_ptr() for p in self.packs])
        self._qflux = ptr_array([p.d_qflux.data_ptr() for p in self.packs])
        L = grid.layout
        keep = []
        qs = [_face_spec(neumann.get(f) if neumann is not None else None, L, keep) for f in FACES]
        self._has_q = any(q[0] != _lib.FACE_NONE for q in qs)
        self._q_args = ((ctypes.c_int * 6)(*[q[0] for q in qs]), (ctypes.c_double * 6)(*[q[1] for q in qs]),
                        ptr_array([q[2].data_ptr() if q[2] is not None else None for q in qs]), keep)
        self._h_none = ((ctypes.c_int * 6)(*[_lib.FACE_NONE] * 6), (ctypes.c_double * 6)(), ptr_array([None] * 6))
        if T is not None:
            self.rebuild(T)

    def _launch(self, T, Tinf, k0, k1, full):
        g, m = self.grid, self.mat
        t = _native_f64(g, T)                                 # host arrays / foreign tensors: a copy (not the step's path)
        law = self.loss.as_c(self.Tinf if Tinf is None else Tinf)
        check(lib.adi_surface_loss_update(ctypes.byref(law), float(self.Tinf if Tinf is None else Tinf), _p(t), _p(g.d_flags),
                                          _p(g.d_bricks), *g.layout.pd, g.dx, m.rho, m.cp, self._coeff, int(k0), int(k1),
                                          int(full), _stream()))

    def update(self, T, Tinf=None):
        """the per-step mode over the whole box, from the device field T (DeviceField or tensor in the grid's layout);
        Tinf: the step's ambient (default: the one given at construction)"""
        self._launch(T, Tinf, 0, self.grid.layout.pz, 0)
        return self.packs

    def rebuild(self, T, k_begin=0, k_end=None, Tinf=None):
        """the full mode on the planes [k_begin, k_end) of axis 2 (clipped to the box), for the grid's CURRENT mask"""
        g, m = self.grid, self.mat
        whole = k_end is None and int(k_begin) <= 0
        k0 = max(0, int(k_begin))
        k1 = g.layout.pz if whole else min(g.nz, g.nz if k_end is None else int(k_end))
        if k1 > k0:
            if self._has_q:
                hm, hs, hf = self._h_none
                qm, qs, qf, _ = self._q_args
                check(lib.adi_build_coeffs_planes(_p(g.d_mask), *g.layout.pd, g.dx, m.rho, m.cp, hm, hs, hf, qm, qs, qf,
                                                  self._coeff, self._qflux, k0, min(k1, g.layout.pz), _stream()))
            self._launch(T, Tinf, k0, k1, 1)
        for a, p in enumerate(self.packs):
            p.mask_version = g.mask_version
            p._fractions = (g, a, g.mask_version)
        return self.packs


# ---- latent heat of melting and freezing (include/adi_hip.h) -----------------------------------------
class PhaseChange:
    """Latent heat `latent_heat` [J/kg] released between `T_solidus` and `T_liquidus` (the field's unit), linearly in T: on
    the equilibrium curve the liquid fraction is f_eq(T) = min(max((T - Ts)/(Tl - Ts), 0), 1).  The step runs at constant cp
    from the state (T, f); afterwards the cell's enthalpy cp*T + L*f is put back on the curve (temperature recovery: lagged,
    first order in dt).  `correct` is the definition, adi_phase_apply the same operations on the device."""

    def __init__(self, latent_heat, T_solidus, T_liquidus):
        self.latent_heat, self.T_solidus, self.T_liquidus = latent_heat, T_solidus, T_liquidus
        self.validate()

    def validate(self):
        """ValueError for anything adi_phase_change rejects (include/adi_hip.h).  -> (L, Ts, Tl) as floats"""
        try:
            L, Ts, Tl = float(self.latent_heat), float(self.T_solidus), float(self.T_liquidus)
        except (TypeError, ValueError):
            raise ValueError("PhaseChange: latent_heat, T_solidus and T_liquidus must be real numbers")
        if not (np.isfinite(L) and np.isfinite(Ts) and np.isfinite(Tl)):
            raise ValueError("PhaseChange: non-finite parameter")
        if not L > 0.0:
            raise ValueError("PhaseChange: latent_heat must be > 0")
        if not Tl > Ts:
            raise ValueError("PhaseChange: T_liquidus must be above T_solidus")
        return L, Ts, Tl

    def as_c(self):
        return _lib.PhaseChangeLaw(*self.validate())

    def key(self):
        """every parameter of the law: a launch takes it by value, so a captured graph holds the law of its capture"""
        return self.validate()

    def constants(self, cp):
        """(dT, Hs, Hl, cm) for heat capacity cp, each one fp64 operation, as the library's host code evaluates them"""
        L, Ts, Tl = self.validate()
        cp = float(cp)
        if not (np.isfinite(cp) and cp > 0.0):
            raise ValueError("PhaseChange: cp must be finite and > 0")
        dT = Tl - Ts
        Hs = cp * Ts
        h1 = cp * Tl
        Hl = h1 + L
        r = L / dT
        cm = cp + r
        return dT, Hs, Hl, cm

    def f_eq(self, T):
        """the liquid fraction on the equilibrium curve at temperatures T (ndarray)"""
        _, Ts, Tl = self.validate()
        T = np.asarray(T, dtype=np.float64)
        dT = Tl - Ts
        e = T - Ts
        x = e / dT
        x = np.where(x < 0.0, 0.0, x)
        return np.where(x > 1.0, 1.0, x)

    def correct(self, T_star, f, mask, dir_mask, cp):
        """(T, f) after the correction of the step's result T_star from the liquid fraction f it started with: THE DEFINITION
        of the law -- one fp64 operation per line, in the order the kernel performs them.  mask: the grid's mask; dir_mask: the
        Dirichlet cells (None: none).  Off-mask cells, Dirichlet cells and cells at rest keep T_star and f bit for bit."""
        L, Ts, Tl = self.validate()
        dT, Hs, Hl, cm = self.constants(cp)
        cp = float(cp)
        Tst = np.asarray(T_star, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64)
        act = np.asarray(mask, dtype=bool)
        if dir_mask is not None:
            act = act & ~np.asarray(dir_mask, dtype=bool)
        rest = ((f == 0.0) & (Tst <= Ts)) | ((f == 1.0) & (Tst >= Tl))
        act = act & ~rest
        h1 = cp * Tst
        h2 = L * f
        H = h1 + h2
        # H <= Hs: all solid
        Ta = H / cp
        # H >= Hl: all liquid
        d1 = H - L
        Tb = d1 / cp
        # between: on the mushy branch of the curve
        d2 = H - Hs
        q = d2 / cm
        Tc = Ts + q
        e = Tc - Ts
        x = e / dT
        x = np.where(x < 0.0, 0.0, x)
        fc = np.where(x > 1.0, 1.0, x)
        lo, hi = H <= Hs, H >= Hl
        Tn = np.where(lo, Ta, np.where(hi, Tb, Tc))
        fn = np.where(lo, 0.0, np.where(hi, 1.0, fc))
        return np.where(act, Tn, Tst), np.where(act, fn, f)


class _SeededForMask:
    """What PhaseField and ThermalHistory share: a per-cell state seeded for one version of `self.grid`'s mask, the mask then
    seen, and the re-seed of the cells that joined the mask since.  `seed(T, sel)` is the owner's and ends in _remember_mask."""
    _seen = None                 # the device mask at the last seed (None: never seeded)
    _mask_version = None

    def _remember_mask(self):
        self._seen = self.grid.d_mask.clone()
        self._mask_version = self.grid.mask_version

    def sync_mask(self, T):
        """after a mask change: the cells that joined the mask since the last seed / sync are seeded from T, those that left it
        are cleared (the seed does that off the mask), every other cell keeps its state; never seeded: every in-mask cell"""
        g = self.grid
        if g.mask_version != self._mask_version:
            self.seed(T, sel=None if self._seen is None else (g.d_mask != 0) & (self._seen == 0))


class PhaseField(_SeededForMask):
    """The liquid fraction of a grid under a PhaseChange law, on the device: `f` (fp64, the grid's layout, 0 off the mask) and
    the phase summary (one word per 16^3 brick, 0 exactly when every f of the brick is 0: adi_phase_apply far from the melt
    pool reads T once and nothing else).  Both buffers live as long as the object, so a StagedStepper's graph holds their
    pointers.  T (optional): the field f is seeded from, f = f_eq(T) on the mask; without it everything is solid.
    dir_mask (optional): the Dirichlet cells of `apply` calls that are not given any (the step passes its pack's).
        apply(T)              the correction on a device field in the grid's layout, T and f in place: one launch
        seed(T, sel=None)     f = f_eq(T) on the in-mask cells `sel` selects (None: all), 0 off the mask
        sync_mask(T)          after `grid.mask` changed: the cells that joined the mask are seeded from T, those that left it
                              are zeroed, every other cell keeps its f
        snapshot() / restore(s), copy_state_from(other)     f and the summary"""

    def __init__(self, grid, mat, law, T=None, dir_mask=None):
        if not isinstance(law, PhaseChange):
            raise TypeError("PhaseField: law must be a PhaseChange")
        law.constants(mat.cp)
        self.grid, self.mat, self.law = grid, mat, law
        L = grid.layout
        self._flat = torch.zeros(L.numel_padded, dtype=torch.float64, device=_device())
        self.f = self._flat.as_strided(L.shape, L.strides)
        self.summary = torch.zeros(self._words(), dtype=torch.int32, device=_device())
        self.d_dir_mask = None if dir_mask is None else L.to_layout(dir_mask, torch.uint8)
        if T is not None:
            self.seed(T)
        else:
            self._remember_mask()

    def _words(self):
        n = int(lib.adi_phase_summary_words(*self.grid.layout.pd[:3]))
        if n <= 0:
            raise ValueError("PhaseField: bad grid")
        return n

    @property
    def liquid_fraction(self):
        """a copy of f as a DeviceField of the grid's shape"""
        return DeviceField(self.f).copy()

    def apply(self, T, d_dir_mask=None):
        """adi_phase_apply on T (a DeviceField or device tensor in the grid's layout), in place; d_dir_mask: the Dirichlet
        cells as a uint8 device tensor in the grid's layout (default: the ones given at construction)"""
        g = self.grid
        t = _native_f64(g, T, "PhaseField.apply: T must be a fp64 device field in the grid's layout (it is corrected in place)")
        if g.mask_version != self._mask_version:
            raise ValueError("PhaseField: the grid's mask changed since the liquid fraction was seeded; call sync_mask(T)")
        assert self.summary.numel() == self._words()
        dm = self.d_dir_mask if d_dir_mask is None else d_dir_mask
        if dm is not None:
            assert g.layout.is_native(dm) and dm.dtype == torch.uint8
        check(lib.adi_phase_apply(ctypes.byref(self.law.as_c()), float(self.mat.cp), _p(t), _p(self.f), _p(g.d_flags),
                                  _p(g.d_bricks), _p(dm), _p(self.summary), *g.layout.pd, _stream()))
        return T

    def seed(self, T, sel=None):
        """adi_phase_seed: f = f_eq(T) on the in-mask cells `sel` selects (bool / uint8 array or tensor of the grid's shape;
        None: every in-mask cell), 0 off the mask; the summary is rewritten"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        assert self.summary.numel() == self._words()
        check(lib.adi_phase_seed(ctypes.byref(self.law.as_c()), _p(_native_f64(g, T)), _p(self.f), _p(g.d_flags), _p(g.d_bricks),
                                 _p(d_sel), _p(self.summary), *g.layout.pd, _stream()))
        self._remember_mask()

    def set_liquid_fraction(self, f):
        """load f (array / tensor / DeviceField of the grid's shape; taken as 0 off the mask) and rebuild the summary from it
        on the device: a seed that selects no cell keeps every in-mask f, zeroes the rest and rewrites every entry"""
        g = self.grid
        self.f.copy_(g.layout.to_layout(f, torch.float64))
        self.seed(g.layout.empty(zero=True), sel=g.layout.empty(torch.uint8, zero=True))

    def snapshot(self):
        return self._flat.clone(), self.summary.clone()

    def restore(self, s):
        self._flat.copy_(s[0])
        self.summary.copy_(s[1])

    def copy_state_from(self, other):
        if other.grid.layout.pd != self.grid.layout.pd:
            raise ValueError("PhaseField.copy_state_from: the grids differ in layout")
        self._flat.copy_(other._flat)
        self.summary.copy_(other.summary)

    def graph_key(self):
        """what a captured graph holds of the field: the law by value, the buffers by pointer"""
        return (self.law.key(), self.f.data_ptr(), self.summary.data_ptr(),
                None if self.d_dir_mask is None else self.d_dir_mask.data_ptr())


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


class ThermalHistory(_SeededForMask):
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

    def set_clock(self, dt):
        """the block's clock from the host clock: t0 = .t, this dt, n = 0 (the log slot stays)"""
        check(lib.adi_history_set_clock(_p(self.d_block), self.t, float(dt), _stream()))

    def advance_clock(self, t0, dt, nsteps):
        """host side of `nsteps` recorded steps of dt from t0: their end times join the log's, .t = t0 + nsteps*dt"""
        self._times.extend(t0 + (n + 1) * dt for n in range(nsteps))
        self.t = t0 + nsteps * dt

    def record(self, T_in, T_out, dt):
        """one step T_in (at .t) -> T_out (at .t + dt), both fp64 device fields in the grid's layout: one record launch and the
        tick; afterwards .t = t0 + dt"""
        strict = "ThermalHistory.record: T_in and T_out must be fp64 device fields in the grid's layout"
        t_in, t_out = _native_f64(self.grid, T_in, strict), _native_f64(self.grid, T_out, strict)
        self._check_mask()
        dt = float(dt)
        self.set_clock(dt)
        self._launch_record(t_in, t_out)
        self.advance_clock(self.t, dt, 1)

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


# the reference's backend-specific names, so its drivers run unchanged on this module
adi_step_numba_coeff = adi_step_hip_coeff
adi_step_gpu_coeff = adi_step_hip_coeff


class StagedStepper:
    """The step of adi_step_hip_coeff with its arguments resolved once, for tight loops over a
    device-resident field (drivers call the step `nsub` times with the same packs and dt,
    quick_compare_dirichlet_robin.py:169-178).  `events`: optional list of 5 torch.cuda.Event recorded on
    the launch stream before/between/after the four stage kernels (per-stage HIP-event timing).  With `phase=` (a PhaseField
    of the grid) the latent-heat correction is the last launch of every step, after the last of the five marks: the stage
    times stay those of the stage kernels.  With `history=` (a ThermalHistory of the grid) the record launch and its tick follow,
    the last launches of every step; `run` sets the recorder's block from the recorder's own clock `history.t` (not from `t0`,
    which stays the source's time origin) and moves that clock on by nsteps*dt."""

    def __init__(self, grid, mat, params, packs, Tinf=0.0, fused=None, source=None, surface_loss=None, phase=None,
                 history=None):
        _check_extras(grid, mat, packs, source, surface_loss, phase, history)
        self.grid, self.mat, self.params, self.packs, self.Tinf = grid, mat, params, packs, float(Tinf)
        # temperature-dependent surface loss: the packs' Robin coefficients rewritten from the step's INPUT buffer, the first
        # launch of every step -- captured with it (X -> Y reads X, Y -> X reads Y); the law travels by value in that launch,
        # so its parameters are part of run()'s graph key
        self.surface_loss = surface_loss
        # latent heat: the correction of the step's OUTPUT buffer, the last launch of every step -- captured with it; the law
        # travels by value and f and the summary by pointer, so all three are part of run()'s graph key
        self.phase = phase
        # thermal history: the record of the step input -> output and the tick of its block, the last launches of every step
        # -- captured with it; the levels travel by value and the five buffers by pointer, so all are part of run()'s graph key
        self.history = history
        # moving source: corrected after sweep 0 (adi_source_lines0), its time read from a device block whose step counter
        # a captured tick advances -- power, origin, velocity, eta and f_f may change between runs without a new graph
        self.source = source
        self.captures = 0              # HIP graphs captured by run() so far
        self.fused = fused_supported(grid) if fused is None else (bool(fused) and fused_supported(grid))
        if self.fused:
            # the fused kernel reads T + flags (+ the pack arrays of the axis-0 sweep) and writes U: the sweep's own
            # byte count (SURVEY.md 8(d) variant rule); R0 never reaches HBM
            self.stage_names = ['explicit+sweep_axis0', 'sweep_axis1', 'sweep_axis2_contig']
            self.stage_bytes_per_cell = [p.bytes_per_cell for p in packs]
        else:
            self.stage_names = ['explicit', 'sweep_axis0', 'sweep_axis1', 'sweep_axis2_contig']
            self.stage_bytes_per_cell = [float(_lib.EXPLICIT_BYTES_PER_CELL)] + [p.bytes_per_cell for p in packs]

    def sweep_into(self, axis, t_in, t_out, variant=None, dense=False):
        if variant == _lib.SWEEP_GENERAL:
            _ensure_general(self.packs[axis])
        _sweep_into(axis, t_in, t_out, self.grid, self.mat, self.params, self.packs[axis], self.Tinf, variant,
                    dense=dense)

    def _step_into(self, t, out, captured=True, mark=_no_mark):
        """one step t -> out (both native-layout device tensors), no allocation: what a HIP graph captures"""
        _launch_step(t, out, self.grid, self.mat, self.params, self.packs, self.Tinf, self.fused, source=self.source, owner=self,
                     surface_loss=self.surface_loss, phase=self.phase, history=self.history, captured=captured, mark=mark)

    def run(self, T, nsteps, graph=True, t0=0.0):
        """The drivers' `nsub` loop (quick_compare_dirichlet_robin.py:169-178, waam_from_stl_v7_mm.py:525-528): `nsteps`
        steps with the same packs and dt on a device-resident field, returned as a new DeviceField.  The launches of
        two steps (X -> Y -> X) are captured once into a HIP graph and replayed, so small grids are not bound by the
        host's launch path (64^3: 3 kernels + 3 memsets per step, each a ctypes call); the graph is rebuilt when dt,
        theta, Tinf, the mask or the packs change.  graph=False: plain launches.
        t0: time at the start of the first step (a source's step i runs at t0 + i*dt + dt/2); the source's block is
        written here, so its power / origin / velocity as they are now hold for this run, and a change of its support's
        extent recaptures."""
        g, prm = self.grid, self.params
        nsteps = int(nsteps)
        key = (float(prm.dt), float(prm.theta), self.Tinf, g.mask_version, tuple(id(p) for p in self.packs),
               tuple(getattr(p, 'mask_version', None) for p in self.packs),
               tuple(None if p.d_coeff is None else p.d_coeff.data_ptr() for p in self.packs), self.fused,
               None if self.source is None else self.source.shape_key(),
               None if self.surface_loss is None else self.surface_loss.loss.key(),
               None if self.phase is None else self.phase.graph_key(),
               None if self.history is None else self.history.graph_key())
        if self.history is not None:
            self.history._check_mask()
        st = getattr(self, '_graph', None)
        if st is None or st['key'] != key:
            X, Y = g.layout.empty(), g.layout.empty()
            st = self._graph = dict(key=key, X=X, Y=Y, g=None)
        X, Y = st['X'], st['Y']
        X.copy_(g.layout.to_layout(T, torch.float64))
        if self.source is not None:
            self.source.set_block(_source_block(self), t0, prm.dt)
        if graph and nsteps >= 2 and st['g'] is None:
            g.scratch(2)                                   # every buffer exists before the capture
            stateful = [x for x in (self.phase, self.history) if x is not None]
            held = [x.snapshot() for x in stateful]        # (the warm-up steps would advance f, the history, its log and clock)
            if self.history is not None:
                self.history.set_clock(prm.dt)
            self._step_into(X, Y); self._step_into(Y, X)   # warm-up outside the capture (lazy module loads, and the
            self._step_into(X, Y); self._step_into(Y, X)   # no-fallback promise is learnt on the third step); harmless:
            X.copy_(g.layout.to_layout(T, torch.float64))  # X is restored
            for x, snap in zip(stateful, held):
                x.restore(snap)                            # ... and so is what the extras hold
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                self._step_into(X, Y)
                self._step_into(Y, X)
            st['g'] = cg
            self.captures += 1
        if self.source is not None:
            self.source.set_block(_source_block(self), t0, prm.dt)   # (after the warm-up: the counter starts at 0)
        if self.history is not None:
            self.history.set_clock(prm.dt)                 # (likewise; the recorder's own clock, not t0)
        done = 0
        if graph and st['g'] is not None:
            for _ in range(nsteps // 2):
                st['g'].replay()
            done = 2 * (nsteps // 2)
        cur, oth = X, Y
        for _ in range(nsteps - done):
            self._step_into(cur, oth)
            cur, oth = oth, cur
        if self.history is not None:
            self.history.advance_clock(self.history.t, float(prm.dt), nsteps)
        out = g.layout.empty()
        out.copy_(cur)
        return DeviceField(out)

    def step(self, T, events=None, t=0.0):
        """one step from time t (the source, if any, at t + dt/2)"""
        g, prm = self.grid, self.params
        if self.source is not None:
            self.source.set_block(_source_block(self), t, prm.dt)
        t_in = g.layout.to_layout(T, torch.float64)
        out = g.layout.empty()
        ev = iter(events or ())
        self._step_into(t_in, out, captured=False, mark=(lambda: next(ev).record()) if events else _no_mark)
        return DeviceField(out)
