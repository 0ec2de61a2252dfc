"""CPU: the solidification record of the cylindrical step -- the host twin adi_cyl_solid_record_host (the kernel's per-cell code
compiled for the host) against the NumPy definition CylSolidificationRecord.record_reference, the coverage of the cases, the hot
words, the definition's own physics on three analytic fields, the log's spill row, the argument checks, the margin of the spiral
driver's reference loop and the kernels' footprint.  No GPU."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cyl_solid_cases as sc  # noqa: E402

EPS = np.finfo(np.float64).eps
CASES = sc.case_ids()


def _rec():
    from adi_thermal_fields_amd.cyl_solid import CylSolidificationRecord
    return CylSolidificationRecord


@pytest.fixture(scope='module')
def loops():
    """the reference loop and the host-twin loop of every case, computed once"""
    out = {}
    for shape, mode, r_in in CASES:
        case = sc.make_case(shape, mode)
        grid = sc.Grid(shape, r_in)
        out[(shape, mode)] = (case, grid, sc.reference_loop(case, grid), sc.host_loop(case, grid))
    return out


@pytest.mark.parametrize('c', CASES, ids=sc.case_name)
def test_host_twin_is_the_definition_bit_for_bit(loops, c):
    """(t_solid, cooling_rate, g2) after each of the 6 chained steps and the front rows; cells that never froze stay NaN"""
    case, grid, (ref, ref_log), (host, store, rows, blk) = loops[(c[0], c[1])]
    froze = np.zeros(c[0], bool)
    for n, (r, h) in enumerate(zip(ref, host)):
        for a, b in zip(r['state'], h['state']):
            assert sc.same_values(a, b), n
        act = np.ones(c[0], bool) if r['act'] is None else r['act']
        froze |= act & (r['A'] > sc.T_F) & (r['B'] <= sc.T_F)
    assert froze.any()
    for s in host[-1]['state']:
        assert np.array_equal(np.isnan(s), ~froze)
    assert np.array_equal(rows, ref_log)
    assert (rows[:sc.NSTEPS, 0] > 0).any() and int(blk[3]) == sc.NSTEPS and int(blk[2]) == sc.NSTEPS
    assert (store[:sc.GUARD] == sc.GUARD_WORD).all() and (store[-sc.GUARD:] == sc.GUARD_WORD).all()
    for n, r in enumerate(ref):
        assert int(rows[n, 8:10].copy().view(np.int64)[0]) == r['front']['sum_i'] and rows[n, 0] == r['front']['cells']
        assert rows[n, 7] == 0 and (rows[n, 10:] == 0).all()


def test_the_cases_cover_every_neighbour_situation_the_seam_and_a_refreeze(loops):
    """asserted, not assumed: among the freezing cells of the cases, on each axis, both neighbours / only the lower / only the
    upper / none occur; cells freeze at j = 0 and at j = nphi - 1; some cell freezes twice"""
    seen = [set(), set(), set()]
    seam_lo = seam_hi = refreeze = False
    for (shape, mode), (case, grid, (ref, _), _) in loops.items():
        count = np.zeros(shape, int)
        for r in ref:
            act = np.ones(shape, bool) if r['act'] is None else r['act']
            fz = act & (r['A'] > sc.T_F) & (r['B'] <= sc.T_F)
            for ax, s in enumerate(sc.neighbour_situations(fz, r['act'])):
                seen[ax] |= s
            count += fz
            if shape[1] > 1:
                seam_lo |= bool(fz[:, 0, :].any())
                seam_hi |= bool(fz[:, -1, :].any())
        refreeze |= bool((count >= 2).any())
    for ax in range(3):
        assert seen[ax] == {'both', 'lo', 'hi', 'none'}, (ax, seen[ax])
    assert seam_lo and seam_hi and refreeze


@pytest.mark.parametrize('shape', sc.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_hot_words_give_the_bits_of_the_null_path(loops, shape):
    """the chained `all` case: seeded from the first input and passed to every record, the words change no bit of the state or
    of the rows, and after each step they equal hot_reference of that step's result"""
    Rec = _rec()
    case, grid, (ref, ref_log), (plain, _, _, _) = loops[(shape, 'all')]
    host, store, rows, _ = sc.host_loop(case, grid, hot=True)
    for n, (r, p, h) in enumerate(zip(ref, plain, host)):
        for a, b in zip(p['state'], h['state']):
            assert sc.same_values(a, b), n
        assert np.array_equal(h['hot'], Rec.hot_reference(r['B'], None, sc.T_F, shape)), n
    assert np.array_equal(rows, ref_log)
    _, words = sc.host_hot(shape, 7)
    sc.host_hot_seed(ref[0]['A'], None, words)
    assert np.array_equal(words, Rec.hot_reference(ref[0]['A'], None, sc.T_F, shape))


COLD_SHAPES = [(1, 1, 4000), (1, 1, 3999)]                   # pair form and scalar form, 8 tiles each


def _mostly_cold(shape):
    """a step on one long z line, cold in most tiles: three warm stretches in which cells freeze, two inside a tile, one across
    the tile boundary at 1024.  nr = nphi = 1, so a freezing cell's only neighbours are its z neighbours, and every stretch
    ends well inside a tile whose word is set: no neighbour of a freezing cell lies in a tile whose word is clear (a freezing
    cell does read its neighbours from whichever tile they lie in)"""
    rng = np.random.default_rng(21)
    A = rng.uniform(300.0, 900.0, shape)
    for k0, k1 in ((100, 140), (1000, 1050), (2100, 2130)):
        A[0, 0, k0:k1] = rng.uniform(1430.0, 1480.0, k1 - k0)
    B = A - rng.uniform(5.0, 60.0, shape)
    return np.ascontiguousarray(A), np.ascontiguousarray(B)


@pytest.mark.parametrize('shape', COLD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_clear_tiles_do_not_read_the_input(shape):
    """with the words seeded from A, replacing A by 1e300 in every tile whose word is clear changes no bit"""
    Rec = _rec()
    grid = sc.Grid(shape, 0.03)
    A, B = _mostly_cold(shape)
    hot = Rec.hot_reference(A, None, sc.T_F, shape)
    ntile = len(hot) // shape[0]
    assert list(hot) == [1, 1, 1, 0, 1, 0, 0, 0]
    want, front = Rec.record_reference(sc.nan_state(shape), A, B, None, 1.0, 0.5, grid, sc.T_F)
    assert front['cells'] > 10 and front['lo'][2] < 140 and front['hi'][2] >= 2100
    A2 = A.copy()
    flat = A2.reshape(shape[0], -1)
    for i in range(shape[0]):
        for q in range(ntile):
            if not hot[i * ntile + q]:
                flat[i, q * sc.TILE:(q + 1) * sc.TILE] = 1e300
    for src in (A, A2):
        state = sc.nan_state(shape)
        _, rows = sc.host_log(1)
        _, words = sc.host_hot(shape, 0)
        sc.host_hot_seed(A, None, words)
        assert np.array_equal(words, hot)
        sc.host_record(grid, sc.host_block(1.0, 0.5, 1), src, B, state, rows, None, words)
        for a, b in zip(state, want):
            assert sc.same_values(a, b)
        assert np.array_equal(rows[0], Rec.front_row(front))
        assert np.array_equal(words, Rec.hot_reference(B, None, sc.T_F, shape))


# ---- the definition's own physics --------------------------------------------------------------------------------------------
def _both(grid, A, B, act, t_n, dt, T_f, state=None):
    """one record through the definition and through the twin -> the two states (asserted equal) as one"""
    Rec = _rec()
    state = sc.nan_state(A.shape) if state is None else state
    want, _ = Rec.record_reference(state, A, B, act, t_n, dt, grid, T_f)
    got = tuple(np.ascontiguousarray(s).copy() for s in state)
    _, rows = sc.host_log(1)
    sc.host_record(grid, sc.host_block(t_n, dt, 1), np.ascontiguousarray(A), np.ascontiguousarray(B), got, rows, act, None, T_f)
    for a, b in zip(got, want):
        assert sc.same_values(a, b)
    return want


@pytest.mark.parametrize('r_in', sc.R_INS)
def test_gradient_of_a_field_linear_in_r_and_z_is_the_slope(r_in):
    """T = T_f + 50 + a r + c z, cooled by 200 K in the step: every difference quotient, central or one-sided, is the slope.
    Bar: a field value carries eps/2 |T|, a difference of two eps max|T|, the quotient eps max|T| / h; the two components, their
    interpolation between A and B and the norm add a few more roundings: 4 eps max|T| / min(dr, dz) = 1.4e-9 K/m absolute on
    G = 5.0e3 K/m.  Measured: 4.6e-11 K/m."""
    shape = (5, 4, 9)
    grid = sc.Grid(shape, r_in)
    a, c = 3.0e3, -4.0e3
    z = (np.arange(shape[2]) + 0.5) * grid.dz
    A = np.broadcast_to(sc.T_F + 50.0 + a * grid.r[:, None, None] + c * z[None, None, :], shape).copy()
    B = A - 200.0
    assert (A > sc.T_F).all() and (B <= sc.T_F).all()
    state = _both(grid, A, B, None, 0.0, 0.1, sc.T_F)
    G = np.sqrt(state[2])
    err = float(np.max(np.abs(G - math.hypot(a, c))))
    bar = 4 * EPS * float(np.max(np.abs(A))) / min(grid.dr, grid.dz)
    print('max |G - slope| = %.3g K/m, bar %.3g' % (err, bar))
    assert err <= bar


@pytest.mark.parametrize('r_in', sc.R_INS)
def test_gradient_of_c_sin_phi_is_the_central_quotient(r_in):
    """T = T_f + 250 + c sin(phi_j), cooled by 500 K: g_phi = c cos(phi_j) sin(dphi) / (dphi r_i) exactly for the central
    difference over the periodic seam.  Bar: the quotient's eps max|T| / h with h = r_0 dphi, the smallest step, times 4 as
    above -- absolute, because cos(phi) passes near 0: 4 eps max|T| / (r_0 dphi) = 8.5e-9 K/m at R_in = 0.  Measured: 4.7e-10 K/m
    (1.2e-15 of the largest G)."""
    shape = (4, 16, 3)
    grid = sc.Grid(shape, r_in)
    c = 200.0
    phi = (np.arange(shape[1]) + 0.5) * grid.dphi
    A = np.broadcast_to(sc.T_F + 250.0 + c * np.sin(phi)[None, :, None], shape).copy()
    B = A - 500.0
    assert (A > sc.T_F).all() and (B <= sc.T_F).all()
    state = _both(grid, A, B, None, 0.0, 0.1, sc.T_F)
    G = np.sqrt(state[2])
    want = np.abs(c * np.cos(phi)[None, :, None] * math.sin(grid.dphi) / (grid.dphi * grid.r[:, None, None]))
    err = float(np.max(np.abs(G - want)))
    bar = 4 * EPS * float(np.max(np.abs(A))) / (grid.r[0] * grid.dphi)
    print('max |G - exact| = %.3g K/m (%.3g of max G), bar %.3g' % (err, err / float(np.max(want)), bar))
    assert err <= bar


def test_planar_front_gives_its_time_and_speed():
    """T = T_f + G0 (z - v t) over 200 steps: a cell freezes at t_solid = z / v, and R = cooling_rate / G = v.  T is linear in
    t, so the interpolation is exact and only rounding remains.  With e = eps max|T|: num = A - T_f errs by e against
    den = G0 v dt, so t_solid by dt e / den = e / (G0 v), plus the clock's eps t; the rate den / dt errs by e / dt relative to
    G0 v, G by e / dz relative to G0.  Bars, 4 times each: |t_solid - z/v| <= 4 (e / (G0 v) + eps t) = 2.3e-14 s at the end;
    |R/v - 1| <= 4 e (1 / (G0 v dt) + 1 / (G0 dz)) = 3.5e-13.  Measured: 1.8e-15 s and 3.1e-14."""
    shape = (2, 3, 64)
    grid = sc.Grid(shape, 0.03, dz=1.0e-3)
    G0, v, dt, T_f = 1.0e5, 5.0e-3, 0.05, sc.T_F
    z = (np.arange(shape[2]) + 0.5) * grid.dz
    field = lambda t: np.broadcast_to(T_f + G0 * (z - v * t)[None, None, :], shape).copy()   # noqa: E731
    state = sc.nan_state(shape)
    Tmax = float(np.max(np.abs(field(0.0))))
    for n in range(200):
        state = _both(grid, field(n * dt), field((n + 1) * dt), None, n * dt, dt, T_f, state)
    done = np.isfinite(state[0])
    assert done[:, :, :49].all() and not done[:, :, 51:].any()
    zz = np.broadcast_to(z[None, None, :], shape)
    e = EPS * Tmax
    err_t = float(np.max(np.abs(state[0][done] - zz[done] / v)))
    bar_t = 4 * (e / (G0 * v) + EPS * 200 * dt)
    inner = done.copy()
    R = state[1][inner] / np.sqrt(state[2][inner])
    err_R = float(np.max(np.abs(R / v - 1.0)))
    bar_R = 4 * e * (1.0 / (G0 * v * dt) + 1.0 / (G0 * grid.dz))
    print('max |t_solid - z/v| = %.3g s (bar %.3g), max |R/v - 1| = %.3g (bar %.3g)' % (err_t, bar_t, err_R, bar_R))
    assert err_t <= bar_t and err_R <= bar_R


def test_spill_row_and_dropped_with_capacity_2():
    """5 steps into a log of 2 rows: rows 0 and 1 hold steps 0 and 1, the spill row collects steps 2 - 4, slot = 5 (3 dropped),
    the guard words either side are intact"""
    Rec = _rec()
    shape = (5, 8, 129)
    case = sc.make_case(shape, 'births')
    grid = sc.Grid(shape)
    ref, _ = sc.reference_loop(case, grid)
    store, rows = sc.host_log(2)
    blk = sc.host_block(sc.T0_CLOCK, sc.DT, 2)
    state = sc.nan_state(shape)
    want = np.tile(sc.EMPTY_ROW, (3, 1))
    for n in range(5):
        sc.host_record(grid, blk, ref[n]['A'], ref[n]['B'], state, rows, ref[n]['act'])
        sc.merge_row(want[min(n, 2)], Rec.front_row(ref[n]['front']))
    assert np.array_equal(rows, want)
    assert want[2, 0] == sum(ref[n]['front']['cells'] for n in (2, 3, 4)) > 0
    assert int(blk[3]) == 5 and max(0, int(blk[3]) - 2) == 3
    assert (store[:sc.GUARD] == sc.GUARD_WORD).all() and (store[-sc.GUARD:] == sc.GUARD_WORD).all()
    for a, b in zip(state, ref[4]['state']):
        assert sc.same_values(a, b)


def test_argument_errors_without_gpu():
    """every check comes before any HIP call"""
    from adi_thermal_fields_amd._lib import lib, check
    p = [ctypes.c_void_p(64 * (i + 1)) for i in range(9)]
    geo = (sc.T_F, 0.0, 1e-3, 0.1, 1e-3)
    nan, inf = float('nan'), float('inf')
    for fn, tail in ((lib.adi_cyl_solid_record, (None,)), (lib.adi_cyl_solid_record_host, ())):
        def call(geo=geo, blk=p[0], a=p[1], b=p[2], ts=p[3], cr=p[4], g2=p[5], log=p[6], dims=(2, 2, 2, 0)):
            check(fn(*geo, blk, a, b, ts, cr, g2, log, None, None, *dims, *tail))
        for kw in (dict(blk=None), dict(a=None), dict(b=None), dict(ts=None), dict(cr=None), dict(g2=None), dict(log=None)):
            with pytest.raises(ValueError, match='null argument'):
                call(**kw)
        with pytest.raises(ValueError, match='T_out aliases T_in'):
            call(b=p[1])
        for kw in (dict(ts=p[1]), dict(cr=p[2]), dict(g2=p[1])):
            with pytest.raises(ValueError, match='a state array aliases T'):
                call(**kw)
        for kw in (dict(cr=p[3]), dict(g2=p[3]), dict(g2=p[4])):
            with pytest.raises(ValueError, match='the state arrays alias'):
                call(**kw)
        for tf in (nan, inf):
            with pytest.raises(ValueError, match='T_freeze not finite'):
                call(geo=(tf,) + geo[1:])
        for k in (2, 3, 4):
            for bad in (0.0, -1.0, nan, inf):
                with pytest.raises(ValueError, match='must be positive'):
                    call(geo=geo[:k] + (bad,) + geo[k + 1:])
        for bad in (-1e-9, nan, inf):
            with pytest.raises(ValueError, match='R_in must be >= 0'):
                call(geo=(geo[0], bad) + geo[2:])
        with pytest.raises(ValueError, match='8-byte aligned'):
            call(log=ctypes.c_void_p(68))
        with pytest.raises(ValueError, match='8-byte aligned'):
            call(blk=ctypes.c_void_p(68))
        with pytest.raises(ValueError, match='bad grid'):
            call(dims=(2, 0, 2, 0))
        with pytest.raises(ValueError, match='more than 65535 radii'):
            call(dims=(70000, 2, 2, 0))
        with pytest.raises(ValueError, match='plane_stride'):
            call(dims=(2, 2, 2, 3))
        with pytest.raises(ValueError, match='plane too large'):
            call(dims=(2, 65536, 65536, 0))
    for fn, tail in ((lib.adi_cyl_solid_hot_seed, (None,)), (lib.adi_cyl_solid_hot_seed_host, ())):
        with pytest.raises(ValueError, match='null argument'):
            check(fn(sc.T_F, None, None, p[1], 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='null argument'):
            check(fn(sc.T_F, p[0], None, None, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='hot aliases T'):
            check(fn(sc.T_F, p[0], None, p[0], 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='T_freeze not finite'):
            check(fn(nan, p[0], None, p[1], 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='bad grid'):
            check(fn(sc.T_F, p[0], None, p[1], 2, 2, -1, 0, *tail))


def test_python_argument_errors_without_gpu():
    """the wrong type is a TypeError, an object built for another grid a ValueError: both before anything touches the GPU"""
    from adi_thermal_fields_amd import adi3d_hip_cyl as hc
    g1 = hc.GridCyl(2, 3, 4, 1e-3, 0.1, 1e-3, 2e-3)
    g2 = hc.GridCyl(2, 3, 4, 1e-3, 0.1, 1e-3, 2e-3)
    mat, prm, zbc, wall = hc.Material(7800.0, 500.0, 30.0), hc.Params(0.1, 1.0, 'be'), hc.ZBC(), hc.RobinR(0.0, 0.0)
    for bad in ('x', None, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='T_freeze'):
            hc.CylSolidificationRecord(g1, bad)
    with pytest.raises(ValueError, match='capacity'):
        hc.CylSolidificationRecord(g1, 1400.0, capacity=0)
    with pytest.raises(TypeError, match='solidification must be a CylSolidificationRecord'):
        hc.adi_step(np.zeros(g1.shape), g1, mat, prm, wall, zbc, solidification=1400.0)
    with pytest.raises(TypeError, match='solidification must be a CylSolidificationRecord'):
        hc.adi_step_masked(np.zeros(g1.shape), g1, mat, prm, wall, zbc, np.ones(g1.shape, bool), solidification=1400.0)
    with pytest.raises(TypeError, match='solidification must be a CylSolidificationRecord'):
        hc.StagedCylStepper(g1, mat, prm, wall, zbc, solidification=1400.0)

    class _Fake(hc.CylSolidificationRecord):
        def __init__(self, grid):
            self.grid = grid
    with pytest.raises(ValueError, match='solidification was built for another grid'):
        hc.adi_step(np.zeros(g1.shape), g1, mat, prm, wall, zbc, solidification=_Fake(g2))
    with pytest.raises(ValueError, match='solidification was built for another grid'):
        hc.StagedCylStepper(g1, mat, prm, wall, zbc, solidification=_Fake(g2))
    assert hc.__all__[-1] == 'CylSolidificationRecord' and hc.CylSolidificationRecord._keyword == 'solidification'
    from adi_thermal_fields_amd import waam
    from oracle import cyl_oracle
    import cyl_extras_cases as cc
    with pytest.raises(ValueError, match='needs the device loop'):
        waam.run_spiral_deposition(cyl_oracle, *cc.spiral_args(), solidification=1400.0)
    with pytest.raises(ValueError, match='needs the device loop'):
        waam.run_spiral_deposition(hc, *cc.spiral_args(), solidification=1400.0, device_resident=False)


def test_spiral_reference_stays_clear_of_the_freezing_level():
    """the reference loop of the driver test, alone: no compared A or B within 1e-6 relative of T_freeze = 1400 at any step (so
    the GPU test's tolerance on the fields cannot flip a comparison), all 96 deposited cells freeze, over 25 of the 40 steps,
    and the smallest A - B at a crossing is 8 K.  Measured margin: 9.0e-4."""
    ref = sc.spiral_solid_reference()
    print('margin %.3g, steps with a freezing cell %d, smallest drop %.3g K' % (ref['margin'], ref['froze_steps'], ref['min_drop']))
    assert ref['margin'] > 1e-6
    froze = np.isfinite(ref['state'][0])
    s = sc.cc.SPIRAL
    deposited = ref['masks'][-1].copy()
    deposited[:, :, :int(round(s['z_back'] / s['layer_h']))] = False
    assert len(ref['rows']) == 40 and int(deposited.sum()) == 96
    assert np.array_equal(froze, deposited)
    assert ref['froze_steps'] == 25 and ref['min_drop'] >= 8.0
    assert sum(int(r[0]) for r in ref['rows']) >= 96


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_abi_version_stays():
    from adi_thermal_fields_amd import _lib
    for name in ('adi_cyl_solid_record', 'adi_cyl_solid_record_host', 'adi_cyl_solid_hot_seed', 'adi_cyl_solid_hot_seed_host'):
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.adi_abi_version() == 18 and _lib.CYL_SOLID_TILE == sc.TILE == 512
    with open(os.path.join(ROOT, 'include', 'adi_hip.h')) as f:
        text = f.read()
    assert re.search(r'#define ADI_CYL_SOLID_TILE 512\b', text) and re.search(r'#define ADI_ABI_VERSION 18\b', text)


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    ks = [k for k in kernel_meta.all_kernels() if k['obj'] == 'adi_cyl_solid.o']
    names = {re.match(r'(?:void )?adi::(\w+)', k['short']).group(1) for k in ks}
    assert names == {'k_cyl_solid_record', 'k_cyl_solid_hot_seed'} and len(ks) == 4
    for k in ks:
        print('%-40s %3d VGPRs %3d SGPRs %4d B LDS %d B scratch' % (k['short'], k['vgpr_count'], k['sgpr_count'], k['lds'],
                                                                    k['scratch']))
    bad = ['%s: %d B scratch, %d spilled VGPRs' % (k['short'], k['scratch'], k.get('vgpr_spill_count', 0))
           for k in ks if k['scratch'] != 0 or k.get('vgpr_spill_count', 0) != 0]
    assert not bad, '\n'.join(bad)
    # LDS: the front reduction of the record kernel (4 waves x 5 words) and the word per thread the workgroup's votes take
    assert all(k['lds'] <= 4 * 5 * 4 + 256 for k in ks)
