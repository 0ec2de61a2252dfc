"""CPU: latent heat and thermal history of the cylindrical step -- the host twins of the two kernels (adi_cyl_phase_apply_host,
adi_cyl_history_record_host: the kernels' per-cell code compiled for the host) against the NumPy definitions
CylPhaseField.apply_reference and CylThermalHistory.record_reference, the definitions' own physics (enthalpy per cell, heat
content of an adiabatic cylinder under the oracle's step), the argument checks and the kernels' footprint.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cyl_extras_cases as cc  # noqa: E402

EPS = np.finfo(np.float64).eps
CASES = cc.case_ids()
SKIPS = [(True, False), (False, True), (True, True)]


@pytest.fixture(scope='module')
def loops():
    """the reference loop and the host-twin loop of every case, computed once"""
    out = {}
    for shape, mode, r_in in CASES:
        case = cc.make_case(shape, mode)
        out[(shape, mode)] = (case, cc.reference_loop(case), cc.host_loop(case))
    return out


@pytest.mark.parametrize('c', CASES, ids=cc.case_name)
def test_host_twins_are_the_definitions_bit_for_bit(loops, c):
    """(T, f) and (T_peak, t_hi, t_lo) after each of the 6 steps: newborn seeding, NaN kept on inactive cells, steps that cross
    both levels at once"""
    case, (ref, _), (host, _, _, _) = loops[(c[0], c[1])]
    both = 0
    for n, (r, h) in enumerate(zip(ref, host)):
        assert cc.same_bits(r['T'], h['T']), n
        assert cc.same_values(r['f'], h['f']), n
        for a, b in zip(r['state'], h['state']):
            assert cc.same_values(a, b), n
        act = np.ones(c[0], bool) if case['acts'][n] is None else case['acts'][n]
        T_hi, T_lo, _ = cc.LEVEL_ARGS
        both += int(np.count_nonzero(act & (r['A'] > T_hi) & (r['T'] <= T_lo)))
        if case['acts'][n] is not None:                                       # inactive cells: never written
            off = ~case['acts'][n]
            assert cc.same_bits(h['T'][off], r['A'][off])
            assert np.isnan(h['f'][off]).all() and all(np.isnan(s[off]).all() for s in h['state'])
    assert both > 0, 'no step of this case crosses both levels at once'
    last = ref[-1]
    assert np.isfinite(last['state'][1]).any() and np.isfinite(last['state'][2]).any()
    assert ((last['f'] > 0.0) & (last['f'] < 1.0)).any() and (last['f'] == 1.0).any() and (last['f'] == 0.0).any()


@pytest.mark.parametrize('c', CASES, ids=cc.case_name)
def test_log_rows_are_integer_equal(loops, c):
    _, (ref, ref_log), (_, store, rows, blk) = loops[(c[0], c[1])]
    assert np.array_equal(rows, ref_log)
    assert (rows[:cc.NSTEPS, 0] > 0).any() and int(blk[3]) == cc.NSTEPS and int(blk[2]) == cc.NSTEPS
    assert (store[:cc.GUARD] == cc.GUARD_WORD).all() and (store[-cc.GUARD:] == cc.GUARD_WORD).all()
    for n, r in enumerate(ref):
        sum_i = int(rows[n, 8:10].copy().view(np.int64)[0])
        assert sum_i == r['pool']['sum_i'] and rows[n, 0] == r['pool']['cells']
        assert rows[n, 7] == 0 and (rows[n, 10:] == 0).all()


@pytest.mark.parametrize('skip', SKIPS)
@pytest.mark.parametrize('shape,mode', [((3, 5, 7), 'births'), ((2, 1, 36), 'random'), ((5, 8, 129), 'all')])
def test_skipped_dirichlet_planes_are_never_written(shape, mode, skip):
    case = cc.make_case(shape, mode, seed=3, skip=skip)
    ref, _ = cc.reference_loop(case)
    host, _, _, _ = cc.host_loop(case)
    planes = [k for k, on in zip((0, shape[2] - 1), skip) if on]
    for n, (r, h) in enumerate(zip(ref, host)):
        assert cc.same_bits(r['T'], h['T']) and cc.same_values(r['f'], h['f']), n
        f_before = host[n - 1]['f'] if n else cc._start(case)[1]
        for k in planes:
            assert cc.same_bits(h['T'][:, :, k], cc._t_star(case, n, r['A'])[:, :, k])
            assert cc.same_values(h['f'][:, :, k], f_before[:, :, k])
    moved = [not cc.same_bits(host[-1]['T'][:, :, k], case['T0'][:, :, k]) for k in range(1, shape[2] - 1)]
    assert any(moved)


def test_spill_row_and_dropped_with_capacity_2():
    """5 steps into a log of 2 rows: rows 0 and 1 hold steps 0 and 1, the spill row collects steps 2 - 4, slot = 5 (3 dropped),
    the guard words either side are intact"""
    case = cc.make_case((5, 8, 129), 'births')
    law, levels = cc.objects()
    ref, _ = cc.reference_loop(case)
    from adi_thermal_fields_amd.cyl_extras import CylThermalHistory
    store, rows = cc.host_log(2)
    blk = cc.host_block(cc.T0_CLOCK, cc.DT, 2)
    state = tuple(np.full(case['shape'], np.nan) for _ in range(3))
    want = np.tile(cc.EMPTY_ROW, (3, 1))
    for n in range(5):
        cc.host_history_record(levels, blk, np.ascontiguousarray(ref[n]['A']), np.ascontiguousarray(ref[n]['T']), state, rows,
                               case['acts'][n])
        cc.merge_row(want[min(n, 2)], CylThermalHistory.pool_row(ref[n]['pool']))
    assert np.array_equal(rows, want)
    assert want[2, 0] == sum(ref[n]['pool']['cells'] for n in (2, 3, 4)) > 0
    assert int(blk[3]) == 5 and max(0, int(blk[3]) - 2) == 3
    assert (store[:cc.GUARD] == cc.GUARD_WORD).all() and (store[-cc.GUARD:] == cc.GUARD_WORD).all()
    for a, b in zip(state, ref[4]['state']):
        assert cc.same_values(a, b)


@pytest.mark.parametrize('r_in', cc.R_INS)
def test_pool_volume_is_the_sum_of_the_cell_volumes(r_in):
    """volume = dphi dz dr ((R_in + dr/2) cells + dr sum_i) against sum r_i dr dphi dz over the pool cells: 4 eps64"""
    from adi_thermal_fields_amd.adi3d_hip_cyl import GridCyl
    from adi_thermal_fields_amd.cyl_extras import CylThermalHistory
    shape = (5, 8, 129)
    g = GridCyl(*shape, 0.0013, 2.0 * np.pi / shape[1], 0.0021, r_in + shape[0] * 0.0013, R_in=r_in)
    case = cc.make_case(shape, 'random')
    ref, log = cc.reference_loop(case)
    for n, r in enumerate(ref):
        pool_cells = (case['acts'][n]) & (r['T'] >= cc.LEVEL_ARGS[2])
        want = float(np.sum(np.broadcast_to(g.r[:, None, None], shape)[pool_cells] * g.dr * g.dphi * g.dz))
        got = CylThermalHistory.pool_volume(g, log[n, 0], log[n, 8:10].copy().view(np.int64)[0])
        assert want > 0.0
        # the sum of `cells` rounded terms drifts by about sqrt(cells) eps; it is taken in long double so that the bar is the formula's
        exact = float(np.sum((np.broadcast_to(g.r[:, None, None], shape)[pool_cells].astype(np.longdouble)
                              * np.longdouble(g.dr) * np.longdouble(g.dphi) * np.longdouble(g.dz))))
        assert abs(got - exact) <= 4 * EPS * exact, (got, exact, want)


@pytest.mark.parametrize('c', CASES[:6], ids=cc.case_name)
def test_correction_keeps_each_cells_enthalpy(loops, c):
    """cp T + L f of every corrected cell before and after: at most four rounded operations lie between H and (T, f), so
    8 eps64 |H|"""
    case, (ref, _), _ = loops[(c[0], c[1])]
    law, _ = cc.objects()
    L = law.validate()[0]
    worst = 0.0
    f_prev = cc._start(case)[1]
    for n, r in enumerate(ref):
        act = np.ones(c[0], bool) if case['acts'][n] is None else case['acts'][n]
        f0 = np.where(act & np.isnan(f_prev), law.f_eq(r['A']), f_prev)
        H0 = cc.CP * cc._t_star(case, n, r['A'])[act] + L * f0[act]
        H1 = cc.CP * r['T'][act] + L * r['f'][act]
        worst = max(worst, float(np.max(np.abs(H1 - H0) / np.abs(H0))) / EPS)
        f_prev = r['f']
    print('largest |dH| / |H| = %.2f eps' % worst)
    assert worst <= 8.0


@pytest.mark.parametrize('r_in', cc.R_INS, ids=['cylinder', 'annulus'])
def test_adiabatic_cylinder_conserves_heat_through_melting(r_in):
    """h = 0 on the wall, neumann0 at both ends: the oracle's step plus the definition conserve sum r_i (cp T + L f), 10 steps
    each at dt = 0.003, 0.03 and 0.3 s from T uniform in [1200, 1650] around Ts = 1400, Tl = 1450: 1e-12 relative (the sweeps
    conserve sum r_i T to rounding, the correction each cell's enthalpy to a few eps)"""
    from oracle import cyl_oracle as cyl
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField
    law, _ = cc.objects()
    L = law.validate()[0]
    nr, nphi, nz = 6, 64 if r_in == 0.0 else 12, 5
    dr = 1.0e-3
    grid = cyl.GridCyl(nr, nphi, nz, dr, 2.0 * np.pi / nphi, 1.2e-3, r_in + nr * dr, R_in=r_in)
    mat = cyl.Material(7800.0, cc.CP, 30.0)
    wall, zbc = cyl.RobinR(0.0, 25.0), cyl.ZBC(kind_bot='neumann0', kind_top='neumann0')
    rng = np.random.default_rng(11)
    T = rng.uniform(1200.0, 1650.0, (nr, nphi, nz))
    f = law.f_eq(T)
    r = np.asarray(grid.r)[:, None, None]
    heat = lambda T, f: float(np.sum((r * (cc.CP * T + L * f)).astype(np.longdouble)))       # noqa: E731
    worst = 0.0
    for dt in (0.003, 0.03, 0.3):
        prm = cyl.Params(dt, 1.0, "be")
        for _ in range(10):
            H0 = heat(T, f)
            Tst = cyl.adi_step(T, grid, mat, prm, wall, zbc)
            T, f = CylPhaseField.apply_reference(Tst, f, T, None, None, law, cc.CP)
            worst = max(worst, abs(heat(T, f) - H0) / abs(H0))
    print('largest relative change of the heat content over a step: %.3g' % worst)
    assert ((f > 0.0) & (f < 1.0)).any()
    assert worst <= 1e-12


def test_argument_errors_without_gpu():
    """every check comes before any HIP call: null pointers, d_f aliasing d_T, state arrays aliasing fields, bad extents"""
    from adi_thermal_fields_amd import _lib
    from adi_thermal_fields_amd._lib import lib, check
    law, levels = cc.objects()
    lw, lv = ctypes.byref(law.as_c()), ctypes.byref(levels.as_c())
    p = [ctypes.c_void_p(64 * (i + 1)) for i in range(8)]
    for fn, tail in ((lib.adi_cyl_phase_apply, (None,)), (lib.adi_cyl_phase_apply_host, ())):
        with pytest.raises(ValueError, match='null argument'):
            check(fn(lw, cc.CP, None, p[1], None, None, 0, 0, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='f aliases T'):
            check(fn(lw, cc.CP, p[0], p[0], None, None, 0, 0, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='T_in aliases'):
            check(fn(lw, cc.CP, p[0], p[1], p[0], None, 0, 0, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='T_in is required'):
            check(fn(lw, cc.CP, p[0], p[1], None, p[2], 0, 0, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='bad grid'):
            check(fn(lw, cc.CP, p[0], p[1], None, None, 0, 0, 2, 0, 2, 0, *tail))
        with pytest.raises(ValueError, match='plane_stride'):
            check(fn(lw, cc.CP, p[0], p[1], None, None, 0, 0, 2, 2, 2, 3, *tail))
        with pytest.raises(ValueError, match='cp must be'):
            check(fn(lw, -1.0, p[0], p[1], None, None, 0, 0, 2, 2, 2, 0, *tail))
    for fn, tail in ((lib.adi_cyl_history_record, (None,)), (lib.adi_cyl_history_record_host, ())):
        with pytest.raises(ValueError, match='null argument'):
            check(fn(lv, p[0], p[1], p[2], p[3], p[4], None, p[6], None, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='T_out aliases T_in'):
            check(fn(lv, p[0], p[1], p[1], p[3], p[4], p[5], p[6], None, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='a state array aliases T'):
            check(fn(lv, p[0], p[1], p[2], p[2], p[4], p[5], p[6], None, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='the state arrays alias'):
            check(fn(lv, p[0], p[1], p[2], p[3], p[3], p[5], p[6], None, 2, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='bad grid'):
            check(fn(lv, p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, 2, 2, -1, 0, *tail))
        with pytest.raises(ValueError, match='more than 65535 radii'):
            check(fn(lv, p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, 70000, 2, 2, 0, *tail))
        with pytest.raises(ValueError, match='8-byte aligned'):
            check(fn(lv, p[0], p[1], p[2], p[3], p[4], p[5], ctypes.c_void_p(68), None, 2, 2, 2, 0, *tail))
    bad = _lib.HistoryLevelsC(500.0, 800.0, 1450.0)
    with pytest.raises(ValueError, match='T_hi must be above T_lo'):
        check(lib.adi_cyl_history_record(ctypes.byref(bad), p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, 2, 2, 2, 0, None))
    with pytest.raises(ValueError, match='null argument'):
        check(lib.adi_cyl_phase_seed(lw, None, p[1], None, None, 2, 2, 2, 0, None))
    with pytest.raises(ValueError, match='the state arrays alias'):
        check(lib.adi_cyl_history_seed(p[0], p[1], p[1], p[2], None, None, 2, 2, 2, 0, None))
    with pytest.raises(ValueError, match='capacity'):
        check(lib.adi_cyl_history_reset_log(p[0], p[1], 0, None))


def test_python_argument_errors_without_gpu():
    """the wrong type is a TypeError, an object built for another grid a ValueError: both before anything touches the GPU"""
    from adi_thermal_fields_amd import adi3d_hip_cyl as hc
    g1 = hc.GridCyl(2, 3, 4, 1e-3, 0.1, 1e-3, 2e-3)
    g2 = hc.GridCyl(2, 3, 4, 1e-3, 0.1, 1e-3, 2e-3)
    mat, prm, zbc = hc.Material(7800.0, 500.0, 30.0), hc.Params(0.1, 1.0, 'be'), hc.ZBC()
    law, levels = cc.objects()
    with pytest.raises(TypeError, match='law must be a PhaseChange'):
        hc.CylPhaseField(g1, mat, levels)
    with pytest.raises(TypeError, match='levels must be a HistoryLevels'):
        hc.CylThermalHistory(g1, law)
    with pytest.raises(ValueError, match='capacity'):
        hc.CylThermalHistory(g1, levels, capacity=0)
    with pytest.raises(TypeError, match='phase must be a CylPhaseField'):
        hc.adi_step(np.zeros(g1.shape), g1, mat, prm, hc.RobinR(0.0, 0.0), zbc, phase=law)
    with pytest.raises(TypeError, match='history must be a CylThermalHistory'):
        hc.adi_step_masked(np.zeros(g1.shape), g1, mat, prm, hc.RobinR(0.0, 0.0), zbc, np.ones(g1.shape, bool), history=levels)

    class _Fake(hc.CylPhaseField):
        def __init__(self, grid):
            self.grid = grid
    with pytest.raises(ValueError, match='phase was built for another grid'):
        hc.adi_step(np.zeros(g1.shape), g1, mat, prm, hc.RobinR(0.0, 0.0), zbc, phase=_Fake(g2))
    assert set(['CylPhaseField', 'CylThermalHistory', 'PhaseChange', 'HistoryLevels']) <= set(hc.__all__)
    from adi_thermal_fields_amd import waam
    with pytest.raises(ValueError, match='needs the device loop'):
        from oracle import cyl_oracle
        waam.run_spiral_deposition(cyl_oracle, *cc.spiral_args(), phase_change=law)


def test_spiral_reference_stays_clear_of_every_level():
    """the reference loop of the driver test, alone: no compared value within 1e-6 relative of the level it is compared with,
    at any step -- so the GPU test's tolerances cannot hide a flipped comparison -- and the run melts, freezes and cools
    through both levels"""
    from adi_thermal_fields_amd.phase import PhaseChange
    from adi_thermal_fields_amd.history import HistoryLevels
    ref = cc.spiral_reference(PhaseChange(*cc.SPIRAL_LAW), HistoryLevels(*cc.SPIRAL_LEVELS))
    print('smallest relative distance from a level: %.3g' % ref['margin'])
    assert ref['margin'] > 1e-6
    cells = [int(r[0]) for r in ref['rows']]
    print('steps %d, pool cells per step %s' % (len(cells), cells))
    assert len(cells) == 40 and max(cells) > 0 and cells[-1] == 0
    assert np.isfinite(ref['state'][1]).any() and np.isfinite(ref['state'][2]).any()
    assert (ref['f'][ref['masks'][-1]] == 0.0).all() and np.isnan(ref['f'][~ref['masks'][-1]]).all()


# ---- the kernels' footprint ----------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    ks = [k for k in kernel_meta.all_kernels() if k['obj'] == 'adi_cyl_extras.o']
    names = {re.match(r'(?:void )?adi::(\w+)', k['short']).group(1) for k in ks}
    assert names == {'k_cyl_phase_apply', 'k_cyl_history_record', 'k_cyl_phase_seed', 'k_cyl_history_seed',
                     'k_cyl_history_reset_log'} and len(ks) == 7
    for k in ks:
        print('%-40s %3d VGPRs %3d SGPRs %4d B LDS %d B scratch' % (k['short'], k['vgpr_count'], k['sgpr_count'], k['lds'],
                                                                    k['scratch']))
    bad = ['%s: %d B scratch, %d spilled VGPRs' % (k['short'], k['scratch'], k.get('vgpr_spill_count', 0))
           for k in ks if k['scratch'] != 0 or k.get('vgpr_spill_count', 0) != 0]
    assert not bad, '\n'.join(bad)
    # LDS: the log reduction of the record kernel (4 waves x 5 words) and the word per thread the workgroup's votes take
    assert all(k['lds'] <= (4 * 5 * 4 + 256 if 'record' in k['short'] else 0) for k in ks)
