"""CPU: the definition of the step on a grid of several materials (MaterialMap.step_reference / packs_reference / pair_table_of,
NumPy fp64) against the extended-precision reference tests/matmap_ref_ld.py and against the physics it stands for; the C ABI's
argument checks; the new kernels' footprint.  Cases, metric and bar: tests/matmap_cases.py.  No GPU."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import matmap_cases as mc
import matmap_ref_ld
from adi_thermal_fields_amd import _lib
from adi_thermal_fields_amd.packs import MaterialMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _definition(c, **kw):
    return mc.run(MaterialMap.step_reference, MaterialMap.packs_reference, c, **kw)


# ---- the bar ----------------------------------------------------------------------------------------------------------------
def test_recorded_worst_ulp_is_the_measured_one():
    small = [k for k in mc.keys() if k[5] <= 1e-3]
    assert len(small) >= 4
    worst = 0.0
    for k in small:
        f = mc.figures(_definition(mc.case(k)), k)
        print('%-70s %.3f ulp' % (mc.tag(k), f['ulp']))
        worst = max(worst, f['ulp'])
    print('worst %.3f, recorded %.3f, A_MAP %g' % (worst, mc.MAP_WORST_ULP, mc.A_MAP))
    assert worst <= mc.MAP_WORST_ULP <= 2.0 * worst
    assert mc.A_MAP == mc.bar_factor(mc.MAP_WORST_ULP) == 16.0


@pytest.mark.parametrize(**mc.params(lambda k: k[0] in ('holes', 'past_limit', 'rows16') or (k[0] == 'layers' and k[2][2] in (1, 8))))
def test_definition_meets_the_bar(key):
    c = mc.case(key)
    ok, f = mc.meets_bar(_definition(c), c, mc.reference(key))
    assert ok, (mc.tag(key), f)


# ---- physics ----------------------------------------------------------------------------------------------------------------
def _adiabatic(shape, seed, nmat=3):
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) > 0.25
    ids = rng.integers(0, nmat, shape).astype(np.uint8)
    return mask, ids, rng.uniform(20.0, 1500.0, shape)


@pytest.mark.parametrize('cfl', [1e-3, 0.3, 200.0, 1e6])
@pytest.mark.parametrize('theta', [0.5, 1.0])
def test_heat_of_an_adiabatic_body_is_conserved(cfl, theta):
    """no boundary terms: sum C_i T_i over the mask changes by the rounding of the sum.  kf is symmetric, so the face terms
    cancel pairwise in every stage; what is left is the rounding of ~N additions, N eps64 relative at the very most"""
    shape = (20, 18, 35)
    mask, ids, T0 = _adiabatic(shape, 3)
    dt = cfl * mc.DX ** 2 / mc.ALPHA_MAX
    pk = MaterialMap.packs_reference(mask, ids, mc.MATERIALS, mc.DX)
    W = MaterialMap.step_reference(T0, mask, ids, mc.MATERIALS, mc.DX, dt, theta, pk, mc.TINF)
    C = np.array([rho * cp for rho, cp, _ in mc.MATERIALS], LD)[np.where(mask, ids, 0)]
    h0 = np.sum((C * T0.astype(LD))[mask])
    h1 = np.sum((C * W.astype(LD))[mask])
    rel = float(abs(h1 - h0) / abs(h0))
    print('cfl %g theta %g: sum C T changes by %.2e of itself' % (cfl, theta, rel))
    assert rel <= int(mask.sum()) * mc.EPS64
    assert not np.array_equal(W, T0) and np.array_equal(W[~mask], T0[~mask])


def _series_profile(n, ids_line, mats, Ta, Tb):
    """cell-centre temperatures of a laminate between Dirichlet cells 0 and n-1: the flux kf(i, i+1) (T_{i+1} - T_i) / dx is the
    same across every face (half-cells in series)"""
    k = np.array([m[2] for m in mats], LD)[ids_line]
    R = np.array([LD(1) / k[i] if ids_line[i] == ids_line[i + 1] else (k[i] + k[i + 1]) / (2 * k[i] * k[i + 1])
                  for i in range(n - 1)], LD)
    J = (LD(Tb) - LD(Ta)) / R.sum()
    return np.concatenate([[LD(Ta)], LD(Ta) + J * np.cumsum(R)])


@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('cfl', [0.3, 200.0, 1e6])
def test_series_resistance_profile_of_a_laminate_is_a_fixed_point(axis, cfl):
    """three layers between two Dirichlet planes, adiabatic sides.  Each of the four stages rounds a cell once or twice around an
    exact fixed point: the explicit stage and each sweep leave at most one rounding of a value <= max|T| in a cell, four half-ulps
    of up to 2 eps64 max|T| in all; the bar is twice that, 4 eps64 max|T| (measured 0.6 - 1.4)"""
    n = 13
    shape = [4, 5, 3]; shape[axis] = n
    ids_line = np.array([0] * 4 + [1] * 5 + [2] * 4, np.uint8)
    bshape = [1, 1, 1]; bshape[axis] = n
    prof = _series_profile(n, ids_line, mc.MATERIALS, 100.0, 900.0).astype(np.float64)
    T0 = np.broadcast_to(prof.reshape(bshape), shape).copy()
    ids = np.broadcast_to(ids_line.reshape(bshape), shape).copy()
    mask = np.ones(shape, bool)
    idx = np.arange(n).reshape(bshape)
    dm = np.broadcast_to((idx == 0) | (idx == n - 1), shape).copy()
    dt = cfl * mc.DX ** 2 / mc.ALPHA_MAX
    pk = MaterialMap.packs_reference(mask, ids, mc.MATERIALS, mc.DX, dir_mask=dm, dir_value=T0)
    W = MaterialMap.step_reference(T0, mask, ids, mc.MATERIALS, mc.DX, dt, 0.5, pk, mc.TINF)
    res = float(np.max(np.abs(W - T0))) / (mc.EPS64 * float(np.max(np.abs(T0))))
    print('axis %d cfl %g: residual %.2f eps64 max|T|' % (axis, cfl, res))
    assert res <= 4.0
    assert np.ptp(prof) > 700.0 and len(set(np.round(np.diff(prof), 6))) >= 3      # three different slopes


def test_equal_ids_and_identical_materials_are_the_plain_material():
    """all ids equal, or different ids of identical materials: the plain step of cart_ref_ld and of the pinned oracle"""
    import cart_ref_ld
    from helpers import run_cart_case
    from oracle import adi_oracle
    key = ('holes', mc.HOLES, 'random3', 'general', 0.5, 200.0)
    c = mc.case(key)
    rho, cp, k = mc.STEEL
    cc = dict(shape=c['shape'], dx=c['dx'], mat=dict(rho=rho, cp=cp, k=k), mask=c['mask'], T0=c['T0'], dt=c['dt'], theta=c['theta'],
              Tinf=c['Tinf'], nsteps=1, births=None, **mc.bc_of(c))
    W = run_cart_case(cart_ref_ld, cc)['T_final']
    O = run_cart_case(adi_oracle, cc)['T_final']
    free = c['mask'] & ~c['dir_mask']
    ref = (W[c['mask']], float(np.max(np.abs(W - c['T0'])[free])), float(np.max(np.abs(W[c['mask']]))))
    f_o = mc.figures_of(O, c, ref)
    ref_o = (O[c['mask']], float(np.max(np.abs(O - c['T0'])[free])), float(np.max(np.abs(O[c['mask']]))))
    for what, mats, ids in (('all ids 0', (mc.STEEL, mc.COPPER), np.zeros(c['shape'], np.uint8)),
                            ('three times steel', (mc.STEEL,) * 3, c['ids'])):
        X = _definition(dict(c, materials=mats, ids=ids))
        ok, f = mc.meets_bar(X, c, ref)
        d = float(np.max(np.abs(X - O)[c['mask']]))
        print('%s: %.2f ulp of the plain reference; %.2e K from the oracle (itself %.2f ulp)' % (what, f['ulp'], d, f_o['ulp']))
        assert ok, (what, f)
        ok_o, fo = mc.meets_bar(X, c, ref_o)               # ... and the same bar against the oracle's own result
        assert ok_o and d == fo['abs_err'], (what, fo)


# two bodies in contact: the interface temperature
CONTACT_FINEST_ERR_LD = 5.84e-5   # K, the long-double reference on the finest grid (measured 5.8376e-05; see the test)


def _contact_error(n, step, packs, dtype):
    """|interface temperature - (e1 T1 + e2 T2) / (e1 + e2)| after t = 5 steps of the coarsest grid (n = 16): a line of n
    cells, steel at T1 on the left half and copper at T2 on the right, adiabatic; dx = 64 mm / n, dt ~ dx^2 (cfl 0.3)"""
    T1, T2 = 1200.0, 300.0
    dx = 0.064 / n
    dt = 0.3 * dx * dx / mc.ALPHA_MAX
    nsteps = 5 * (n // 16) ** 2
    shape = (n, 1, 1)
    mask = np.ones(shape, bool)
    ids = (np.arange(n) >= n // 2).astype(np.uint8).reshape(shape)
    mats = (mc.STEEL, mc.COPPER)
    T = np.where(ids == 0, T1, T2).astype(dtype)
    pk = packs(mask, ids, mats, dx)
    for _ in range(nsteps):
        T = step(T, mask, ids, mats, dx, dt, 0.5, pk, 0.0)
    e1, e2 = (np.sqrt(LD(k) * LD(rho) * LD(cp)) for rho, cp, k in mats)
    want = (e1 * T1 + e2 * T2) / (e1 + e2)
    k1, k2 = LD(mats[0][2]), LD(mats[1][2])
    Ti = (k1 * T[n // 2 - 1, 0, 0] + k2 * T[n // 2, 0, 0]) / (k1 + k2)       # the face value of two half-cells in series
    return float(abs(Ti - want))


def test_interface_temperature_of_two_bodies_in_contact():
    errs = [_contact_error(n, MaterialMap.step_reference, MaterialMap.packs_reference, np.float64) for n in (16, 32, 64)]
    ld = _contact_error(64, matmap_ref_ld.step, matmap_ref_ld.packs, LD)
    print('interface temperature error, n = 16, 32, 64: %s K; long double at 64: %.6e K' % (errs, ld))
    assert errs[1] <= errs[0] / 2 and errs[2] <= errs[1] / 2
    assert ld <= CONTACT_FINEST_ERR_LD <= 1.01 * ld            # the recorded figure is the reference's
    assert errs[2] <= 2 * CONTACT_FINEST_ERR_LD


# ---- mutants ----------------------------------------------------------------------------------------------------------------
def _arithmetic_mean(materials, dx, dt):
    G = np.zeros((8, 8))
    for m, (rho, cp, k) in enumerate(materials):
        for n, (_, _, kn) in enumerate(materials):
            G[m, n] = (0.5 * (k + kn)) * dt / (rho * cp * dx * dx)
    return G


def _neighbours_capacity(materials, dx, dt):
    G = np.zeros((8, 8))
    for m, (_, _, k) in enumerate(materials):
        for n, (rho_n, cp_n, kn) in enumerate(materials):
            kf = k if m == n else 2.0 * k * kn / (k + kn)
            G[m, n] = kf * dt / (rho_n * cp_n * dx * dx)
    return G


TWO_MATERIAL = [k for k in mc.keys() if k[0] == 'layers' and k[2][2] in (8, 9)]


@pytest.mark.parametrize('mutant', [_arithmetic_mean, _neighbours_capacity], ids=['arithmetic_mean', 'neighbours_C'])
def test_mutants_of_the_definition_exceed_the_bar(monkeypatch, mutant):
    assert len(TWO_MATERIAL) == 6 and all(k[5] >= 0.3 for k in TWO_MATERIAL)
    real = MaterialMap.pair_table_of
    for key in TWO_MATERIAL:
        c = mc.case(key)
        assert mc.meets_bar(_definition(c), c, mc.reference(key))[0]
        monkeypatch.setattr(MaterialMap, 'pair_table_of', staticmethod(mutant))
        ok, f = mc.meets_bar(_definition(c), c, mc.reference(key))
        monkeypatch.setattr(MaterialMap, 'pair_table_of', staticmethod(real))
        print('%s %s: %.2e K against a bar of %.2e' % (mutant.__name__, mc.tag(key), f['abs_err'], mc.bar(f, mc.A_MAP)))
        assert not ok and f['abs_err'] > 100 * mc.bar(f, mc.A_MAP)


# ---- the table and the constructor ---------------------------------------------------------------------------------------------
def test_pair_table():
    dt = 3.7e-3
    G = MaterialMap.pair_table_of(mc.MATERIALS, mc.DX, dt)
    assert G.shape == (8, 8) and G.dtype == np.float64 and not G[3:].any() and not G[:, 3:].any()
    W = matmap_ref_ld.pair_table(mc.MATERIALS, mc.DX, dt)
    assert np.max(np.abs(G[:3, :3] - W) / W) <= 2 * mc.EPS64
    for m, (rho, cp, k) in enumerate(mc.MATERIALS):
        assert G[m, m] == (k * dt) / ((rho * cp) * (mc.DX * mc.DX))          # k_m itself, not 2 k k / (k + k)
    k0, k1 = mc.STEEL[2], mc.COPPER[2]
    assert G[0, 1] == (((2.0 * k0) * k1) / (k0 + k1) * dt) / ((mc.STEEL[0] * mc.STEEL[1]) * (mc.DX * mc.DX))
    assert G[0, 1] != G[1, 0] and min(k0, k1) < G[0, 1] / G[0, 0] * k0 < max(k0, k1)
    triples = [types.SimpleNamespace(rho=r, cp=c, k=k) for r, c, k in mc.MATERIALS]
    assert np.array_equal(MaterialMap.pair_table_of(triples, mc.DX, dt), G)


def test_constructor_refusals_come_before_any_launch():
    """a grid stand-in without a device: a check that let the constructor go on would fail on it with another error"""
    shape = (4, 5, 6)
    mask = np.ones(shape, bool); mask[0, 0, 0] = False
    grid = types.SimpleNamespace(shape=shape, mask=mask)
    ids = np.zeros(shape, np.uint8)
    two = (mc.STEEL, mc.COPPER)
    with pytest.raises(ValueError, match='shape'):
        MaterialMap(grid, two, np.zeros((4, 5, 7), np.uint8))
    with pytest.raises(ValueError, match='uint8'):
        MaterialMap(grid, two, np.zeros(shape, np.int32))
    with pytest.raises(ValueError, match='NumPy uint8'):
        MaterialMap(grid, two, [[0]])
    bad = ids.copy(); bad[1, 1, 1] = 2
    with pytest.raises(ValueError, match='id 2'):
        MaterialMap(grid, two, bad)
    with pytest.raises(ValueError, match='9 materials'):
        MaterialMap(grid, (mc.STEEL,) * 9, ids)
    with pytest.raises(ValueError, match='0 materials'):
        MaterialMap(grid, (), ids)
    for broken in ((7800.0, 490.0, 0.0), (-1.0, 490.0, 54.0), (7800.0, float('nan'), 54.0), (7800.0, 490.0, float('inf'))):
        with pytest.raises(ValueError, match='finite and > 0'):
            MaterialMap(grid, (mc.STEEL, broken), ids)
    off = ids.copy(); off[0, 0, 0] = 255                       # an id off the mask is never read: the constructor gets past it
    with pytest.raises(AttributeError):                        # ... and fails on the stand-in, at its first use of the device
        MaterialMap(grid, two, off)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
NEW = ('adi_matmap_build_coeffs', 'adi_matmap_explicit', 'adi_matmap_workspace_bytes', 'adi_matmap_sweep')


def test_header_declares_and_lib_binds_the_new_symbols():
    src = open(os.path.join(ROOT, 'include', 'adi_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % n, code), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n), n
    assert 'kf(m, n) = (2 k_m k_n) / (k_m + k_n)' in src and re.search(r'#define\s+ADI_MATMAP_MAX\s+8\b', src)
    assert _lib.MATMAP_MAX == 8 and _lib.lib.adi_abi_version() == 18


def test_argument_errors_come_back_without_a_gpu():
    p = ctypes.c_void_p(8)
    G = (ctypes.c_double * 64)(*([1.0] * 64))
    C = (ctypes.c_double * 8)(*([1.0] * 8))
    I6, D6 = (ctypes.c_int * 6)(), (ctypes.c_double * 6)()
    out3 = _lib.ptr_array([8, 8, 8])
    lib, check = _lib.lib, _lib.check
    with pytest.raises(ValueError, match='bad axis'):
        check(lib.adi_matmap_sweep(3, 3, p, p, p, p, None, None, None, 4, 4, 4, 0, 2, G, 1.0, 0.5, 0.0, p, None, 0, None))
    with pytest.raises(ValueError, match='null argument'):
        check(lib.adi_matmap_sweep(0, 3, p, p, None, p, None, None, None, 4, 4, 4, 0, 2, G, 1.0, 0.5, 0.0, p, None, 0, None))
    with pytest.raises(ValueError, match='aliases'):
        check(lib.adi_matmap_sweep(2, 3, p, p, p, p, None, None, None, 4, 4, 4, 0, 2, G, 1.0, 0.5, 0.0, p, None, 0, None))
    with pytest.raises(ValueError, match='needs Dirichlet arrays'):
        check(lib.adi_matmap_sweep(2, 0, p, p, p, p, None, None, None, 4, 4, 4, 0, 2, G, 1.0, 0.5, 0.0, ctypes.c_void_p(16), None, 0,
                                   None))
    with pytest.raises(ValueError, match='9 materials'):
        check(lib.adi_matmap_sweep(2, 3, p, p, p, p, None, None, None, 4, 4, 4, 0, 9, G, 1.0, 0.5, 0.0, ctypes.c_void_p(16), None, 0,
                                   None))
    with pytest.raises(ValueError, match='needs a workspace of %d bytes' % (1025 * 16 * 8)):  # 1025 rows: one thread per line
        check(lib.adi_matmap_sweep(0, 3, p, p, p, p, None, None, None, 1025, 4, 4, 0, 2, G, 1.0, 0.5, 0.0, ctypes.c_void_p(16), None,
                                   0, None))
    bad = (ctypes.c_double * 64)(*([1.0] * 64)); bad[1] = float('nan')
    with pytest.raises(ValueError, match=r'pair table entry \[0\]\[1\]'):
        check(lib.adi_matmap_explicit(p, None, p, p, 4, 4, 4, 0, 2, bad, C, 1.0, 0.5, ctypes.c_void_p(16), None))
    with pytest.raises(ValueError, match='bad dt or theta'):
        check(lib.adi_matmap_explicit(p, None, p, p, 4, 4, 4, 0, 2, G, C, 1.0, 1.5, ctypes.c_void_p(16), None))
    with pytest.raises(ValueError, match='C of material 1'):
        check(lib.adi_matmap_build_coeffs(p, p, 4, 4, 4, 0, 1e-3, 2, (ctypes.c_double * 2)(1.0, 0.0), I6, D6, None, I6, D6, None, out3,
                                          out3, None))
    with pytest.raises(ValueError, match='bad face mode'):
        check(lib.adi_matmap_build_coeffs(p, p, 4, 4, 4, 0, 1e-3, 2, C, (ctypes.c_int * 6)(0, 0, 5, 0, 0, 0), D6, None, I6, D6, None,
                                          out3, out3, None))
    b = ctypes.c_size_t(7)
    check(lib.adi_matmap_workspace_bytes(2, 4, 4, 1024, 0, ctypes.byref(b)))
    assert b.value == 0
    check(lib.adi_matmap_workspace_bytes(2, 4, 4, 1025, 0, ctypes.byref(b)))
    assert b.value == 4 * 4 * 1025 * 8
    for axis, dims in ((0, (1024, 4, 4)), (1, (4, 1024, 4))):
        check(lib.adi_matmap_workspace_bytes(axis, *dims, 0, ctypes.byref(b)))
        assert b.value == 0


# ---- the kernels' footprint -----------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    ks = [k for k in kernel_meta.all_kernels() if 'k_matmap_' in k['short']]
    names = {re.match(r'adi::(\w+)', k['short']).group(1) for k in ks}
    assert names == {'k_matmap_build_coeffs', 'k_matmap_explicit', 'k_matmap_sweep_contig', 'k_matmap_sweep_strided',
                     'k_matmap_sweep_lines'}
    assert len(ks) == 2 + 16 + 16 + 4 and all(k['obj'] == 'adi_matmap.o' for k in ks)
    bad = ['%s: %d B scratch, %d spilled VGPRs' % (k['short'], k['scratch'], k.get('vgpr_spill_count', 0))
           for k in ks if k['scratch'] != 0 or k.get('vgpr_spill_count', 0) != 0]
    assert not bad, '\n'.join(bad)
