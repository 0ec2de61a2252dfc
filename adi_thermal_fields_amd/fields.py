"""Device layout and fields of the Cartesian backend: where a grid lives in HBM (`Layout`), a resident field with enough of
the ndarray surface for the reference's drivers (`DeviceField`, `to_device`), the grid with its device mask and neighbour
flags (`Grid3D`), and the small helpers every other module of the package reaches the device through (`_device`, `_stream`,
`_p`).  See adi3d_hip_coeff for the operator surface as a whole."""
import ctypes
import itertools

import numpy as np
import torch

from . import _lib
from ._lib import lib, check


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
