"""Cases, metric and bar of tests/test_matmap_cpu.py and tests/test_matmap_gpu.py: ONE theta-step on a grid of several
materials, measured against the extended-precision reference tests/matmap_ref_ld.py, in the form of tests/cart_dt_cases.py.

Metric, for one step from the same float64 T0, W the long-double result:
    abs_err(X) = max over in-mask cells |X - W|,        inc = max over in-mask non-Dirichlet cells |W - T0|
Bar:  abs_err <= A_MAP eps64 max|W| + 1e-10 inc;  off-mask cells bit-equal to T0, Dirichlet cells bit-equal to dir_value.

A_MAP = bar_factor(MAP_WORST_ULP): MAP_WORST_ULP is the worst abs_err(MaterialMap.step_reference) / (eps64 max|W|) over the
cases here with cfl <= 1e-3, measured on the CPU against the reference alone (tests/test_matmap_cpu.py re-measures it and
holds the recorded value between it and twice it); the factor 4 of bar_factor stands for the segment-tree order of
elimination of the kernels, as in cart_dt_cases.  cfl is taken with the largest diffusivity among the materials."""
import functools
import zlib

import numpy as np

import matmap_ref_ld
from cart_dt_cases import EPS64, bar_factor, bar, figures_of, untouched_exact  # noqa: F401  (the metric is cart_dt_cases')

STEEL = (7800.0, 490.0, 54.0)
COPPER = (8900.0, 385.0, 390.0)
INSULATOR = (2700.0, 900.0, 1.5)
MATERIALS = (STEEL, COPPER, INSULATOR)
ALPHA_MAX = max(k / (rho * cp) for rho, cp, k in MATERIALS)
DX = 1e-3
TINF = 20.0

MAP_WORST_ULP = 4.0                         # measured 3.586 (test_matmap_cpu.py re-measures it): eps64 max|W|, cfl <= 1e-3
A_MAP = bar_factor(MAP_WORST_ULP)

HOLES = (20, 18, 35)
LAYERS = (64, 16, 32)
LONG = ((512, 16, 48), (32, 512, 48), (40, 48, 512))
PAST_LIMIT = ((1040, 8, 16), (8, 1040, 16), (8, 16, 1040))     # served: one thread per line
ROWS16 = ((640, 8, 16), (8, 640, 16), (8, 16, 640))            # 513 - 1024 rows: the segment kernels' 16-row builds


def keys():
    """(family, shape, ids, bc, theta, cfl) of every case; ids: 'random3', ('layers', axis, p), 'shells3', 'zero'"""
    out = []
    for theta in (0.5, 1.0):
        out += [('holes', HOLES, 'random3', 'general', theta, cfl) for cfl in (1e-11, 1e-3, 0.3, 200.0, 1e6)]
    for axis, n in enumerate(LAYERS):
        for p in sorted({p for p in (1, 7, 8, 9, 15, 16, 17, n - 1) if p < n}):
            out.append(('layers', LAYERS, ('layers', axis, p), 'robin_neumann', 0.5, 200.0))
    for shape in LONG:
        out += [('long', shape, 'shells3', 'general' if shape[2] == 512 else 'robin_neumann', 0.5, cfl) for cfl in (0.3, 1e6)]
    out += [('past_limit', shape, 'shells3', 'robin_neumann', 0.5, 0.3) for shape in PAST_LIMIT]
    out += [('rows16', shape, 'shells3', 'general', 0.5, cfl) for shape in ROWS16 for cfl in (0.3, 1e6)]
    return out


def tag(key):
    fam, shape, ids, bc, theta, cfl = key
    ids = ids if isinstance(ids, str) else '%s%d_%d' % ids
    return '%s-%dx%dx%d-%s-%s-theta%g-cfl%g' % ((fam,) + shape + (ids, bc, theta, cfl))


def params(select=lambda key: True):
    ks = [k for k in keys() if select(k)]
    return dict(argnames='key', argvalues=ks, ids=[tag(k) for k in ks])


def _ellipsoid_radius(shape):
    g = np.meshgrid(*[(np.arange(n) + 0.5) / n - 0.5 for n in shape], indexing='ij')
    return np.sqrt((g[0] / 0.47) ** 2 + (g[1] / 0.49) ** 2 + (g[2] / 0.48) ** 2)


@functools.lru_cache(maxsize=None)
def _static(fam, shape, ids, bc, theta):
    """everything of a case but the time step; built once, read-only"""
    rng = np.random.default_rng(zlib.crc32(repr((fam, shape, ids, bc, theta)).encode()))
    if fam in ('holes', 'layers'):
        mask = rng.random(shape) > 0.25                   # 25 % random holes
    else:
        mask = _ellipsoid_radius(shape) <= 1.0
    if ids == 'random3':
        idf = rng.integers(0, 3, shape).astype(np.uint8)
    elif ids == 'zero':
        idf = np.zeros(shape, np.uint8)
    elif ids == 'shells3':                                # three concentric shells, 5 % of the cells speckled
        r = _ellipsoid_radius(shape)
        idf = ((r > 0.45).astype(np.uint8) + (r > 0.8).astype(np.uint8)).astype(np.uint8)
        sp = rng.random(shape) < 0.05
        idf[sp] = rng.integers(0, 3, int(sp.sum())).astype(np.uint8)
    else:                                                 # two layers along `axis`, the interface before row p
        _, axis, p = ids
        idx = np.arange(shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)])
        idf = np.broadcast_to((idx >= p).astype(np.uint8), shape).copy()
    mats = MATERIALS if ids in ('random3', 'shells3') else MATERIALS[:2]
    c = dict(shape=shape, dx=DX, materials=mats, mask=mask, ids=idf, T0=rng.uniform(20.0, 1500.0, shape), dir_mask=None,
             dir_value=None, neumann={'z-': 2e5}, robin_h=350.0, Tinf=TINF, theta=theta)
    if bc == 'general':       # per-voxel h on two faces, a flux array on one, 2 % Dirichlet cells in the lowest third
        c['robin_h'] = {'x-': 350.0, 'x+': rng.uniform(20.0, 400.0, shape), 'y-': rng.uniform(20.0, 400.0, shape),
                        'y+': 350.0, 'z-': 350.0, 'z+': 350.0}
        c['neumann'] = {'z-': 2e5, 'y+': rng.uniform(0.0, 1e5, shape)}
        dm = np.zeros(shape, bool)
        low = shape[2] // 3
        dm[:, :, :low] = mask[:, :, :low] & (rng.random((shape[0], shape[1], low)) < 0.02)
        c.update(dir_mask=dm, dir_value=rng.uniform(30.0, 60.0, shape))
    for v in list(c.values()) + list(c['neumann'].values()) + (list(c['robin_h'].values()) if bc == 'general' else []):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(key, dt_factor=1.0):
    fam, shape, ids, bc, theta, cfl = key
    c = dict(_static(fam, shape, ids, bc, theta))
    c['dt'] = dt_factor * cfl * DX * DX / ALPHA_MAX
    return c


def bc_of(c):
    return dict(dir_mask=c['dir_mask'], dir_value=c['dir_value'], neumann=c['neumann'], robin_h=c['robin_h'])


def run(module_step, module_packs, c, T0=None, S=None, return_stages=False):
    """one step of the case dict c by a definition: (matmap_ref_ld.step, matmap_ref_ld.packs) or MaterialMap's pair"""
    pk = module_packs(c['mask'], c['ids'], c['materials'], c['dx'], **bc_of(c))
    return module_step(c['T0'] if T0 is None else T0, c['mask'], c['ids'], c['materials'], c['dx'], c['dt'], c['theta'], pk,
                       c['Tinf'], S=S, return_stages=return_stages)


def reference_of(c, T0=None, S=None):
    """(longdouble values W[mask], inc, max|W|) of one reference step of c; read-only"""
    T0 = c['T0'] if T0 is None else T0
    W = run(matmap_ref_ld.step, matmap_ref_ld.packs, c, T0=T0, S=S)
    mask = c['mask']
    dirc = mask & c['dir_mask'] if c['dir_mask'] is not None else np.zeros_like(mask)
    assert W.dtype == np.longdouble and np.array_equal(W[~mask].astype(np.float64), T0[~mask])
    inc = float(np.max(np.abs(W - T0)[mask & ~dirc]))
    Wm = W[mask]
    Wm.setflags(write=False)
    return Wm, inc, float(np.max(np.abs(Wm)))


@functools.lru_cache(maxsize=None)
def reference(key):
    """reference_of the case of `key`, computed once per session"""
    return reference_of(case(key))


def figures(X, key):
    return figures_of(X, case(key), reference(key))


def meets_bar(X, c, ref, a=None):
    """(ok, figures): the bar and the exactness of the untouched cells"""
    fig = figures_of(X, c, ref)
    return fig['abs_err'] <= bar(fig, A_MAP if a is None else a) and untouched_exact(X, c), fig
