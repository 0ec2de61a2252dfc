"""Inputs of the FieldMonitor tests, shared by the CPU tests (the definition, the census) and the GPU tests (the kernels).
Masks and fields come from seeded generators; every case is small enough for a few seconds."""
import numpy as np

import history_seam_cases as hs

DX, THETA, TINF, H, DT = 1.0e-3, 0.5, 25.0, 40.0, 0.02
RHO, CP, K = 7800.0, 500.0, 30.0
MATERIALS = ((7800.0, 500.0, 30.0), (2700.0, 900.0, 200.0))     # case 4 and the energy test
OFF = 1.0e6          # the value of T off the mask: above every in-mask value, so a cell wrongly included shows
OUTSIDE = 1.0e9      # the value written outside the logical box of a padded layout
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
BRICK = 16
EPS = 2.0 ** -52

# the physical boxes of the padded variants of the GPU tests (None: the layout the library picks)
PADDED = {1: (24, 24, 38), 2: (48, 64, 64)}


def _field(rng, mask):
    T = 300.0 + 700.0 * rng.random(mask.shape)
    return np.where(mask, T, OFF)


def case(n):
    """dict(shape, mask, T0, regions, probes[, ids, extra]); regions as FieldMonitor takes them"""
    rng = np.random.default_rng(7000 + n)
    if n == 1:
        # odd row length: the cell-by-cell loads; bricks cut by the box on every axis
        shape = (23, 19, 37)
        mask = rng.random(shape) < 0.6
        mask[0:3, 0:3, 0:3] = False                       # the empty region
        mask[5, 5, 36] = True                             # a probe on the last cell of an odd row
        mask[6, 6, 6], mask[7, 7, 7] = True, False        # a probe in the mask and one off it
        regions = (None, ((3, 20), (2, 17), (5, 31)), ((17, 20), (17, 19), (33, 36)), ((0, 3), (0, 3), (0, 3)))
        probes = ((6, 6, 6), (7, 7, 7), (5, 5, 36), (22, 18, 36))
    elif n == 2:
        # solid but for a carved corner: all-solid bricks next to flag-reading ones, 16-byte loads; two overlapping regions
        shape = (48, 48, 48)
        mask = np.ones(shape, dtype=bool)
        mask[30:, 35:, 28:] = False
        regions = (((8, 40), (8, 40), (8, 40)), ((20, 48), (30, 48), (10, 44)))
        probes = ((0, 0, 0), (47, 47, 47), (24, 24, 24), (31, 36, 29))
    elif n == 3:
        # 35 bricks along axis 0: a second summary word per brick row
        shape = (560, 48, 48)
        mask = np.ones(shape, dtype=bool)
        mask[500:530, 20:30, 40:] = False
        regions = (None, ((505, 540), (3, 47), (1, 48)))
        probes = ((559, 47, 47), (520, 25, 44), (512, 0, 0))
    elif n == 4:
        shape = (32, 32, 48)
        mask = rng.random(shape) < 0.85
        regions = (None, ((4, 30), (0, 32), (7, 41)))
        probes = ((1, 2, 3),)
    else:
        raise KeyError(n)
    c = dict(shape=shape, mask=mask, T0=_field(rng, mask), regions=regions, probes=probes)
    if n == 4:
        ids = (rng.random(shape) < 0.4).astype(np.uint8)
        c['ids'] = ids
        c['extra'] = np.where(mask, rng.random(shape), OFF)
    return c


CASES = (1, 2, 3, 4)


def boxes(c):
    """the regions of a case as explicit boxes"""
    whole = tuple((0, n) for n in c['shape'])
    return tuple(whole if r is None else r for r in c['regions'])


def phys_of(c, phys=None):
    """the physical box of the case: `phys`, or what the library recommends"""
    if phys is not None:
        return tuple(phys)
    import ctypes
    from adi_thermal_fields_amd import _lib
    a, b, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.adi_recommended_dims(*c['shape'], ctypes.byref(a), ctypes.byref(b), ctypes.byref(d)))
    return a.value, b.value, d.value


def vec_form(c, phys=None):
    """True: the 16-byte loads serve this layout (even row and plane strides; torch allocations are 16-byte aligned)"""
    from adi_thermal_fields_amd import _lib
    p = phys_of(c, phys)
    sx = int(_lib.lib.adi_recommended_plane_stride(p[1], p[2]))
    return p[2] % 2 == 0 and sx % 2 == 0


def solid_bricks(c, phys=None):
    """(nbx, nby, nbz) bool: the bricks the flags summary calls all-solid"""
    return hs.predicted_bricks(c['mask'], phys_of(c, phys))


def region_bricks(box):
    """slices over the brick grid of the bricks a region meets"""
    return tuple(slice(lo // BRICK, (hi - 1) // BRICK + 1) for lo, hi in box)


def setup(mod, c):
    grid = mod.Grid3D(*c['shape'], DX, np.array(c['mask']))
    if 'ids' in c:
        mm = mod.MaterialMap(grid, MATERIALS, np.array(c['ids']), robin_h={f: H for f in FACES})
        return grid, mm.mat, mm.packs, mm
    mat = mod.Material(RHO, CP, K)
    packs = mod.precompute_coeff_packs_unified(grid, mat, robin_h={f: H for f in FACES})
    return grid, mat, packs, None


def reference(FM, c, T, mask=None, regions=None, probes=None, extra=None):
    """record_reference for the case's own regions and probes on the field T"""
    weights = FM.weights_of([_Mat(*m) for m in MATERIALS], DX) if 'ids' in c else None
    return FM.record_reference(T, c['mask'] if mask is None else mask, c['probes'] if probes is None else probes,
                               c['regions'] if regions is None else regions, weights=weights, ids=c.get('ids'),
                               extra=c.get('extra') if extra is None else extra)


class _Mat:
    def __init__(self, rho, cp, k):
        self.rho, self.cp, self.k = rho, cp, k


# ---- directed values --------------------------------------------------------------------------------------------------------
def directed():
    """dict(shape, mask, T, regions, want): fields built by hand, with the extrema each region must log"""
    shape = (20, 36, 40)
    mask = np.ones(shape, dtype=bool)
    mask[10:, 20:, :] = False
    T = np.where(mask, 500.0, OFF)
    regions, want = [], []
    # +0.0 and -0.0 as the only values: the minimum is -0.0, the maximum +0.0, whichever comes first in any order
    T[0:2, 0:2, 0:4] = 0.0
    T[1, 1, 2] = -0.0
    regions.append(((0, 2), (0, 2), (0, 4))); want.append((-0.0, 0.0))
    T[0:2, 4:6, 0:4] = 0.0
    T[0, 4, 0] = -0.0                                     # (the first cell in the order this time)
    regions.append(((0, 2), (4, 6), (0, 4))); want.append((-0.0, 0.0))
    T[4:6, 0:2, 0:4] = -0.0                               # only -0.0
    regions.append(((4, 6), (0, 2), (0, 4))); want.append((-0.0, -0.0))
    T[4:6, 4:6, 0:4] = 0.0                                # only +0.0
    regions.append(((4, 6), (4, 6), (0, 4))); want.append((0.0, 0.0))
    # equal maxima (and minima) in different bricks
    T[3, 17, 3], T[19, 3, 37], T[3, 3, 20] = 900.0, 900.0, 900.0
    T[18, 18, 18], T[2, 30, 2] = 100.0, 100.0
    regions.append(None); want.append((-0.0, 900.0))
    regions.append(((2, 20), (2, 36), (1, 40))); want.append((0.0, 900.0))   # (of the zeros only +0.0 lies inside)
    # one cell
    T[9, 19, 39] = 123.25
    regions.append(((9, 10), (19, 20), (39, 40))); want.append((123.25, 123.25))
    return dict(shape=shape, mask=mask, T=T, regions=tuple(regions), want=want, probes=((9, 19, 39), (1, 1, 2), (15, 25, 5)))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)
