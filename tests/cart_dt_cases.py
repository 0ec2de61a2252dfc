"""Cases, metric and bar of tests/test_cart_ref_cpu.py and tests/test_cart_increment_gpu.py: ONE Cartesian theta-step over the
range of time steps, measured against the extended-precision reference tests/cart_ref_ld.py.  Reference-free.

Why not rel_linf: max|got - want| / max|want| is relative to the field (~1500 K).  At gamma = alpha dt/dx^2 <= 1e-9 a step
changes the field by less than 1e-10 of that, so rel_linf <= 1e-10 passes a step computed with a time step 1 % off, and at
gamma <= 1e-11 it passes a kernel that returns its input (tests/test_cart_ref_cpu.py pins both).

Metric, for one step from the same float64 T0, W the long-double result:
    abs_err(X) = max over in-mask cells |X - W|,        inc = max over in-mask non-Dirichlet cells |W - T0|
Bar:  abs_err <= A eps64 max|W| + 1e-10 inc  -- the rounding floor of a float64 result plus BASELINE.json's 1e-10, taken of
the change the step made instead of the field; off-mask cells bit-equal to T0, Dirichlet cells bit-equal to dir_value.

A is measured, on the CPU, against the references alone: ORACLE_WORST_ULP is the worst abs_err(oracle) / (eps64 max|W|) over
all cases here with cfl <= 1e-3 (the regime in which 1e-10 inc contributes nothing), and A is 4 times that, rounded up to a
power of two.  The 4: the kernels eliminate the same rows in segments merged by a tree instead of one chain, a different
order of the same operations with an error bound of the same form.  tests/test_cart_ref_cpu.py re-measures the worst value
and holds the recorded one between it and twice it.  The same for the cylindrical step (two steps, the cases of
cyl_switch_cases.dt_params with f <= 1e-3): CYL_ORACLE_WORST_ULP and A_CYL."""
import functools
import zlib

import numpy as np

import cart_ref_ld

STEEL = dict(rho=7800.0, cp=490.0, k=54.0)
ALPHA = STEEL['k'] / (STEEL['rho'] * STEEL['cp'])
DX = 1e-3
TINF = 20.0
EPS64 = float(np.finfo(np.float64).eps)
K_MIXED_MIN_TG = 1e-9                       # csrc/adi_core.hpp, kMixedMinTg: below it the GENERAL kernels take the sweep

ORACLE_WORST_ULP = 4.5                      # measured 4.204 (test_cart_ref_cpu.py re-measures it): eps64 max|W|, cfl <= 1e-3
A = 32.0
CYL_ORACLE_WORST_ULP = 10.0                 # measured 8.164 (test_cyl_ref_cpu.py re-measures it): f <= 1e-3, two steps
A_CYL = 64.0


def bar_factor(worst_ulp):
    """4 x the oracle's worst distance from the long-double result, rounded up to a power of two"""
    return float(2.0 ** np.ceil(np.log2(4.0 * worst_ulp)))


# theta*gamma = kMixedMinTg lies between the third and the fourth value
CFL = {0.5: [1e-13, 1e-11, 1.9e-9, 2.1e-9, 1e-7, 1e-5, 1e-3, 0.3, 200.0, 3e4, 1e6],
       1.0: [1e-13, 1e-11, 0.95e-9, 1.05e-9, 1e-7, 1e-5, 1e-3, 0.3, 200.0, 3e4, 1e6]}

# (kernel family the shape is meant to reach, shape, mask): the existing tests' own smallest shapes for those kernels
SHAPES = [('axis1_fast_32rows', (32, 512, 48), 'ellipsoid'),
          ('axis1_fast_30rows_exact_fit', (32, 480, 48), 'ellipsoid'),
          ('fused_axis0_fast', (512, 16, 48), 'ellipsoid'),
          ('contig_fast', (40, 48, 512), 'ellipsoid'),
          ('fused_tiled_small', (64, 16, 32), 'holes'),
          ('general_odd_nz', (20, 18, 35), 'holes'),
          ('island_segments', (256, 48, 64), 'walls')]
GENERAL_BC = ((32, 512, 48), (40, 48, 512), (20, 18, 35))
THETA_1 = ((32, 512, 48), (64, 16, 32))
# profiles/cart_increment_kernel_trace.txt: below the gate (512, 16, 48) launches the kernel set of (64, 16, 32) -- the larger goes
SAME_KERNELS_AS_A_SMALLER_CASE = {((512, 16, 48), cfl) for cfl in (1e-13, 1e-11, 1.9e-9)}
STAGED = [s for _, s, _ in SHAPES if s != (32, 480, 48)]          # one per kernel family, through StagedStepper.step


def keys():
    """(family, shape, mask, bc, theta, cfl) of every case"""
    out = []
    for fam, shape, mname in SHAPES:
        variants = [('robin_neumann', 0.5)]
        if shape in GENERAL_BC:
            variants.append(('general', 0.5))
        if shape in THETA_1:
            variants.append(('robin_neumann', 1.0))
        for bc, theta in variants:
            out += [(fam, shape, mname, bc, theta, cfl) for cfl in CFL[theta] if (shape, cfl) not in SAME_KERNELS_AS_A_SMALLER_CASE]
    return out


def tag(key):
    fam, shape, mname, bc, theta, cfl = key
    return '%s-%dx%dx%d-%s-theta%g-cfl%g' % ((fam,) + shape + (bc, theta, cfl))


def params(select=lambda key: True):
    ks = [k for k in keys() if select(k)]
    return dict(argnames='key', argvalues=ks, ids=[tag(k) for k in ks])


def _mask(shape, mname):
    if mname == 'ellipsoid':              # test_tiny_time_steps_on_long_lines_crossing_a_curved_surface's
        g = np.meshgrid(*[(np.arange(n) + 0.5) / n - 0.5 for n in shape], indexing='ij')
        return (g[0] / 0.47) ** 2 + (g[1] / 0.49) ** 2 + (g[2] / 0.48) ** 2 <= 1.0
    if mname == 'holes':
        from test_step_forms_gpu import _inputs
        return np.array(_inputs(shape)[0])
    from test_hip_parity import _thin_walls
    return _thin_walls(shape, 1, np.random.default_rng(sum(shape)))


@functools.lru_cache(maxsize=None)
def _static(shape, mname, bc, theta):
    """everything of a case but the time step; built once, read-only"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, mname, bc, theta)).encode()))
    mask = _mask(shape, mname)
    c = dict(shape=shape, dx=DX, mat=dict(STEEL), mask=mask, T0=rng.uniform(20.0, 1500.0, shape), dir_mask=None,
             dir_value=None, neumann={'z-': 2e5}, robin_h=350.0, Tinf=TINF, theta=theta, nsteps=1, births=None)
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
    """the case dict helpers.run_cart_case drives; dt_factor scales the time step (the mutant of the CPU test)"""
    fam, shape, mname, bc, theta, cfl = key
    c = dict(_static(shape, mname, bc, theta))
    c['dt'] = dt_factor * cfl * DX * DX / ALPHA
    return c


def cells(c):
    """(in-mask cells, in-mask Dirichlet cells)"""
    mask = c['mask']
    dirc = mask & c['dir_mask'] if c['dir_mask'] is not None else np.zeros_like(mask)
    return mask, dirc


def reference_of(c):
    """cart_ref_ld after the steps of the case dict c, kept on the in-mask cells only (off the mask the step leaves T0):
    (longdouble values W[mask], inc, max|W|); read-only.  (tests/slab_dt_cases.py measures the slab-decomposed step with it.)"""
    from helpers import run_cart_case
    W = run_cart_case(cart_ref_ld, c)['T_final']
    mask, dirc = cells(c)
    assert W.dtype == np.longdouble and np.array_equal(W[~mask].astype(np.float64), c['T0'][~mask])
    inc = float(np.max(np.abs(W - c['T0'])[mask & ~dirc]))
    Wm = W[mask]
    Wm.setflags(write=False)
    return Wm, inc, float(np.max(np.abs(Wm)))


@functools.lru_cache(maxsize=None)
def dt_reference(key):
    """reference_of the case of `key`, computed once per session"""
    return reference_of(case(key))


def figures_of(X, c, ref):
    """abs_err, inc, max|W| of a float64 result X of the case dict c against ref = reference_of(...), and abs_err in units of
    eps64 max|W| ('ulp') and of inc"""
    Wm, inc, wmax = ref
    X = np.asarray(X)
    assert X.dtype == np.float64
    err = float(np.max(np.abs(X[c['mask']] - Wm)))
    return dict(abs_err=err, inc=inc, wmax=wmax, ulp=err / (EPS64 * wmax), of_inc=err / inc)


def figures(X, key):
    return figures_of(X, case(key), dt_reference(key))


def bar(fig, a):
    return a * EPS64 * fig['wmax'] + 1e-10 * fig['inc']


def untouched_exact(X, c):
    """off-mask cells bit-equal to T0, Dirichlet cells bit-equal to dir_value"""
    mask, dirc = cells(c)
    ok = np.array_equal(X[~mask], c['T0'][~mask])
    if dirc.any():
        ok = ok and np.array_equal(X[dirc], np.broadcast_to(c['dir_value'], X.shape)[dirc])
    return ok


def untouched_cells_are_exact(X, key):
    return untouched_exact(X, case(key))


# ---- the cylinder: the same metric on the sweep of cyl_switch_cases.dt_params (two steps) ----------------------------------
def cyl_figures(X, key):
    import cyl_switch_cases as csc
    W, _ = csc.dt_reference(*key)
    T0 = csc.dt_case(*key)['T0']
    err = float(np.max(np.abs(np.asarray(X, dtype=np.float64) - W)))
    inc = float(np.max(np.abs(W - T0)))
    wmax = float(np.max(np.abs(W)))
    return dict(abs_err=err, inc=inc, wmax=wmax, ulp=err / (EPS64 * wmax), of_inc=err / inc)
