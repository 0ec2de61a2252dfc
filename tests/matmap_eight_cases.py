"""Cases of tests/test_matmap_eight_cpu.py and tests/test_matmap_eight_gpu.py: the step on a grid of several materials with all
EIGHT materials the product serves (ADI_MATMAP_MAX), and at every row count at which the sweep kernels change their build.  Metric,
bar and reference are those of tests/matmap_cases.py: abs_err against tests/matmap_ref_ld.py, abs_err <= A_MAP eps64 max|W| + 1e-10
inc, off-mask cells bit-equal to T0, Dirichlet cells bit-equal to dir_value.

MATERIALS8: the three of matmap_cases, then a titanium alloy, aluminium, tungsten, a nickel alloy and graphite.  Copper keeps the
largest diffusivity, so cfl means what it means there.  All 64 pair-table entries and all eight C = rho cp are pairwise distinct by
a relative gap of at least 1e-4 (test_matmap_eight_cpu.py holds it): an id read with a bit missing, a pair index cut short or a
table read transposed lands on another number.

Families (ids uniform on 0 .. 7 per cell, 25 % random holes, the `general` boundary conditions of matmap_cases._static):
  eight    (20, 18, 35) at theta 0.5 and 1, four cfl, on the padded layout (nx + 1, ny + 2, nz + 3); the ROWS16 and PAST_LIMIT
           shapes at cfl 0.3 and 1e6 on the layout the library picks; the PAST_LIMIT shapes once more on the padded layout
  switch   per axis every length at and around that axis's switches of the row build (SWITCH_LENGTHS), the two other extents
           small, odd and no multiple of 8 -- so the line count is a multiple neither of a tile's lines (8 .. 256) nor of the
           lines of a wave (64 / Lp > 1) -- and, for lengths up to 33, with a product of at least 300: more than one 256-line tile.
           The layout is the logical box itself, so the kernel sees the length the case names.
A key is (family, shape, layout, axis, theta, cfl); layout: 'padded', 'library' or 'exact'; axis: the axis under test or None."""
import functools
import zlib

import numpy as np

import matmap_cases as mc
from matmap_cases import A_MAP, DX, EPS64, TINF, bar, bc_of, figures_of, meets_bar, reference_of, run, untouched_exact  # noqa: F401

MATERIALS8 = mc.MATERIALS + ((4430.0, 526.0, 6.7), (2700.0, 897.0, 237.0), (19300.0, 134.0, 173.0), (8190.0, 435.0, 11.4),
                             (1800.0, 710.0, 24.0))
ALPHA_MAX = max(k / (rho * cp) for rho, cp, k in MATERIALS8)
assert ALPHA_MAX == mc.ALPHA_MAX and len(MATERIALS8) == 8
MIN_GAP = 1e-4

HOLES = mc.HOLES
BRICKS_SHAPE = (32, 32, 64)
SWITCH_LENGTHS = {0: (1, 2, 3, 16, 17, 32, 33, 512, 513, 1024, 1025), 1: (1, 2, 3, 16, 17, 32, 33, 512, 513, 1024, 1025),
                  2: (1, 2, 3, 128, 129, 256, 257, 512, 513, 1024, 1025)}
SIDES_SHORT = (15, 21)            # the other two extents of a line of up to 33 rows: 315 lines
SIDES_LONG = (5, 7, 9)            # ... of a longer line: the two entries that are not the axis's


def pad_dims(nx, ny, nz):
    return nx + 1, ny + 2, nz + 3


def switch_shape(axis, n):
    if n <= 33:
        other = list(SIDES_SHORT)
    else:
        other = [s for a, s in enumerate(SIDES_LONG) if a != axis]
    other.insert(axis, n)
    return tuple(other)


def eight_keys():
    out = []
    for theta in (0.5, 1.0):
        out += [('eight', HOLES, 'padded', None, theta, cfl) for cfl in (1e-11, 0.3, 200.0, 1e6)]
    out += [('eight', shape, 'library', None, 0.5, cfl) for shape in mc.ROWS16 + mc.PAST_LIMIT for cfl in (0.3, 1e6)]
    out += [('eight', shape, 'padded', None, 0.5, cfl) for shape in mc.PAST_LIMIT for cfl in (0.3, 1e6)]
    return out


def switch_keys():
    return [('switch', switch_shape(axis, n), 'exact', axis, 0.5, cfl) for axis in range(3) for n in SWITCH_LENGTHS[axis]
            for cfl in (0.3, 1e6)]


def keys():
    return eight_keys() + switch_keys()


def tag(key):
    fam, shape, layout, axis, theta, cfl = key
    return '%s-%dx%dx%d-%s%s-theta%g-cfl%g' % ((fam,) + shape + (layout, '' if axis is None else '-axis%d' % axis, theta, cfl))


def params(ks):
    return dict(argnames='key', argvalues=ks, ids=[tag(k) for k in ks])


def unique_cases(ks):
    """the keys of `ks` that differ in more than the layout: the host definitions never see a layout"""
    seen, out = set(), []
    for k in ks:
        if _case_id(k) not in seen:
            seen.add(_case_id(k))
            out.append(k)
    return out


def _case_id(key):
    return (key[1], key[4], key[5])


def random8(rng, shape):
    return rng.integers(0, 8, shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _static(shape, theta):
    """everything of a case but the time step: matmap_cases._static's `holes` / `general` case with ids on 0 .. 7; read-only"""
    rng = np.random.default_rng(zlib.crc32(repr(('eight', shape, theta)).encode()))
    mask = rng.random(shape) > 0.25
    idf = random8(rng, shape)
    dm = np.zeros(shape, bool)
    low = shape[2] // 3
    c = dict(shape=shape, dx=DX, materials=MATERIALS8, mask=mask, ids=idf, T0=rng.uniform(20.0, 1500.0, shape), Tinf=TINF,
             theta=theta,
             robin_h={'x-': 350.0, 'x+': rng.uniform(20.0, 400.0, shape), 'y-': rng.uniform(20.0, 400.0, shape), 'y+': 350.0,
                      'z-': 350.0, 'z+': 350.0},
             neumann={'z-': 2e5, 'y+': rng.uniform(0.0, 1e5, shape)})
    dm[:, :, :low] = mask[:, :, :low] & (rng.random((shape[0], shape[1], low)) < 0.02)
    c.update(dir_mask=dm, dir_value=rng.uniform(30.0, 60.0, shape))
    for v in list(c.values()) + list(c['neumann'].values()) + list(c['robin_h'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    assert mask.any() and (mask & ~dm).any()
    return c


def case(key):
    _, shape, _, _, theta, cfl = key
    c = dict(_static(shape, theta))
    c['dt'] = cfl * DX * DX / ALPHA_MAX
    return c


@functools.lru_cache(maxsize=None)
def _reference(cid):
    shape, theta, cfl = cid
    return reference_of(case(('', shape, '', None, theta, cfl)))


def reference(key):
    """matmap_cases.reference_of the case of `key`, computed once per session"""
    return _reference(_case_id(key))


def source_field(key):
    """a source field S [W/m^3] for the case: uniform on [0, 5e10], as tests/test_matmap_gpu.py draws it"""
    return np.random.default_rng(zlib.crc32(repr(('S',) + _case_id(key)).encode())).uniform(0.0, 5e10, key[1])


# ---- coverage of the 64 ordered pairs ---------------------------------------------------------------------------------------------
def pair_counts(c, axis, half=None):
    """how often each ordered pair (own id, id of the in-mask upper neighbour along `axis`) occurs on free cells, as 64 counts at
    index own * 8 + upper; half = 0 / 1: only rows r along the axis with r % 16 < 8 / >= 8 (the two words of a 16-row segment)"""
    mask = c['mask']
    free = mask & ~(c['dir_mask'] if c['dir_mask'] is not None else np.zeros_like(mask))
    lo = [slice(None)] * 3; hi = [slice(None)] * 3
    lo[axis] = slice(None, -1); hi[axis] = slice(1, None)
    lo, hi = tuple(lo), tuple(hi)
    sel = free[lo] & mask[hi]
    if half is not None:
        r = np.arange(c['shape'][axis] - 1).reshape([-1 if a == axis else 1 for a in range(3)])
        sel = sel & (((r % 16) >= 8) == bool(half))
    idf = c['ids'].astype(np.intp)
    return np.bincount((idf[lo] * 8 + idf[hi])[sel], minlength=64)


# ---- bricks8: the id pattern of the latent-heat and monitor tests -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bricks8():
    """(mask, ids) on 32 x 32 x 64 = 2 x 2 x 4 bricks of 16^3, brick b = (bi 2 + bj) 4 + bk as the kernels number them:
    brick b < 8 holds id b alone, full for even b and with 25 % holes for odd b; bricks 8 .. 15 hold ids uniform on 0 .. 7 with
    25 % holes, but brick 11, which has no in-mask cell"""
    rng = np.random.default_rng(88)
    shape = BRICKS_SHAPE
    mask = rng.random(shape) > 0.25
    ids = random8(rng, shape)
    for b in range(16):
        bi, bj, bk = b // 8, (b // 4) % 2, b % 4
        sl = (slice(16 * bi, 16 * bi + 16), slice(16 * bj, 16 * bj + 16), slice(16 * bk, 16 * bk + 16))
        if b < 8:
            ids[sl] = b
            if b % 2 == 0:
                mask[sl] = True
        elif b == 11:
            mask[sl] = False
    mask.setflags(write=False)
    ids.setflags(write=False)
    return mask, ids
