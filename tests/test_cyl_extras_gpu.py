"""GPU: latent heat and thermal history of the cylindrical step -- the kernels adi_cyl_phase_apply and adi_cyl_history_record
against the NumPy definitions and their host twins, bit for bit, on every case of cyl_extras_cases.py; what they must never
write; the keywords of adi_step / adi_step_masked; StagedCylStepper.run against step(); run_spiral_deposition against the
reference loop (the oracle's adi_step_masked, then the two definitions)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cyl_extras_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cc.case_ids()
MAT = (7800.0, cc.CP, 30.0)


@pytest.fixture(scope='module')
def hc():
    import torch
    assert torch.cuda.is_available()
    import adi_thermal_fields_amd.adi3d_hip_cyl as hipcyl
    return hipcyl


def _grid(hc, shape, r_in=0.0, dr=1.0e-3, dz=1.2e-3):
    nr, nphi, nz = shape
    return hc.GridCyl(nr, nphi, nz, dr, 2.0 * math.pi / nphi, dz, r_in + nr * dr, R_in=r_in)


def _dev(g, a):
    import torch
    return g.layout.to_layout(np.ascontiguousarray(a), torch.float64)


def _host(hc, t):
    return np.asarray(hc.DeviceField(t))


def _objects(hc, g, case, capacity=cc.NSTEPS):
    """the CylPhaseField and CylThermalHistory of a case, in the state cyl_extras_cases._start gives the reference loop"""
    law, levels = cc.objects()
    a0 = case['acts'][0]
    if case['mode'] == 'births':
        a0 = np.zeros(case['shape'], dtype=bool)               # nothing has been seen active yet
    ph = hc.CylPhaseField(g, hc.Material(*MAT), law, active=a0)
    hist = hc.CylThermalHistory(g, levels, capacity=capacity, t=cc.T0_CLOCK)
    return ph, hist


def _log(hist):
    n = cc.LOG_INTS
    store = hist._log_store.cpu().numpy()
    return store, store[cc.GUARD:cc.GUARD + (hist.capacity + 1) * n].reshape(hist.capacity + 1, n)


@pytest.mark.parametrize('c', CASES, ids=cc.case_name)
def test_kernels_are_the_definitions_and_the_host_twins_bit_for_bit(hc, c):
    shape, mode, r_in = c
    case = cc.make_case(shape, mode)
    ref, ref_log = cc.reference_loop(case)
    host, _, host_rows, _ = cc.host_loop(case)
    g = _grid(hc, shape, r_in)
    ph, hist = _objects(hc, g, case)
    for n in range(cc.NSTEPS):
        act = case['acts'][n]
        a = _dev(g, ref[n]['A'])
        ts = _dev(g, cc._t_star(case, n, ref[n]['A']))
        ph.apply(ts, T_in=a, active=act)
        hist.record(a, ts, cc.DT, active=act)
        got_T, got_f = _host(hc, ts), _host(hc, ph.f)
        for want in (ref[n], host[n]):
            assert cc.same_bits(got_T, want['T']), n
            assert cc.same_values(got_f, want['f']), n
            for s, w in zip((hist.d_peak, hist.d_t_hi, hist.d_t_lo), want['state']):
                assert cc.same_values(_host(hc, s), w), n
        if act is not None:                                     # the NaN of a cell never seen active is the canonical one
            assert cc.same_bits(got_f[~act], np.full(shape, np.nan)[~act])
    store, rows = _log(hist)
    assert np.array_equal(rows, ref_log) and np.array_equal(rows, host_rows)
    assert (store[:cc.GUARD] == cc.GUARD_WORD).all() and (store[-cc.GUARD:] == cc.GUARD_WORD).all()
    assert hist.slot == cc.NSTEPS and hist.t == cc.T0_CLOCK + cc.NSTEPS * cc.DT
    pool = hist.melt_pool()
    assert np.array_equal(pool['cells'], ref_log[:cc.NSTEPS, 0]) and pool['dropped'] == 0
    for n in range(cc.NSTEPS):
        act = np.ones(shape, bool) if case['acts'][n] is None else case['acts'][n]
        cells = act & (ref[n]['T'] >= cc.LEVEL_ARGS[2])
        want = float(np.sum(np.broadcast_to(g.r[:, None, None], shape)[cells].astype(np.longdouble) * np.longdouble(g.dr)
                            * np.longdouble(g.dphi) * np.longdouble(g.dz)))
        assert abs(pool['volume'][n] - want) <= 4 * np.finfo(np.float64).eps * want
        assert pool['t'][n] == cc.T0_CLOCK + (n + 1) * cc.DT
    lf = np.asarray(ph.liquid_fraction)
    assert cc.same_values(lf, np.nan_to_num(ref[-1]['f'], nan=0.0))


@pytest.mark.parametrize('skip', [(True, False), (False, True), (True, True)])
def test_skipped_planes_on_the_device(hc, skip):
    shape = (5, 8, 129)
    case = cc.make_case(shape, 'births', seed=3, skip=skip)
    ref, _ = cc.reference_loop(case)
    g = _grid(hc, shape, 0.03)
    ph, _ = _objects(hc, g, case)
    for n in range(cc.NSTEPS):
        a, ts = _dev(g, ref[n]['A']), _dev(g, cc._t_star(case, n, ref[n]['A']))
        ph.apply(ts, T_in=a, active=case['acts'][n], skip_k0=skip[0], skip_kN=skip[1])
        assert cc.same_bits(_host(hc, ts), ref[n]['T']) and cc.same_values(_host(hc, ph.f), ref[n]['f']), n


def test_capacity_2_spill_row_and_dropped(hc):
    from adi_thermal_fields_amd.cyl_extras import CylThermalHistory
    shape = (5, 8, 129)
    case = cc.make_case(shape, 'births')
    ref, _ = cc.reference_loop(case)
    g = _grid(hc, shape)
    _, hist = _objects(hc, g, case, capacity=2)
    want = np.tile(cc.EMPTY_ROW, (3, 1))
    for n in range(5):
        hist.record(_dev(g, ref[n]['A']), _dev(g, ref[n]['T']), cc.DT, active=case['acts'][n])
        cc.merge_row(want[min(n, 2)], CylThermalHistory.pool_row(ref[n]['pool']))
    store, rows = _log(hist)
    assert np.array_equal(rows, want)
    assert (store[:cc.GUARD] == cc.GUARD_WORD).all() and (store[-cc.GUARD:] == cc.GUARD_WORD).all()
    pool = hist.melt_pool()
    assert pool['dropped'] == 3 and len(pool['cells']) == 2 and hist.slot == 5
    hist.reset(_dev(g, ref[0]['A']), t=0.5, active=case['acts'][0])
    assert hist.slot == 0 and np.array_equal(_log(hist)[1], np.tile(cc.EMPTY_ROW, (3, 1))) and hist.t == 0.5
    a0 = case['acts'][0]
    assert cc.same_values(_host(hc, hist.d_peak), np.where(a0, ref[0]['A'], np.nan))
    assert np.isnan(_host(hc, hist.d_t_hi)).all() and np.isnan(_host(hc, hist.d_t_lo)).all()


@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 3, 1030)])
def test_nothing_is_written_on_inactive_cells(hc, shape):
    """sentinels in T, f and the three state fields on the inactive cells, through one step of both kernels"""
    import torch
    case = cc.make_case(shape, 'random', seed=5)
    act = case['acts'][0]
    ref, _ = cc.reference_loop(case)
    g = _grid(hc, shape)
    ph, hist = _objects(hc, g, case)
    d_off = g.layout.to_layout(~act, torch.uint8) != 0
    for t in (ph.f, hist.d_peak, hist.d_t_hi, hist.d_t_lo):
        t[d_off] = cc.SENTINEL_F
    a, ts = _dev(g, ref[0]['A']), _dev(g, cc._t_star(case, 0, ref[0]['A']))
    assert (_host(hc, ts)[~act] == cc.SENTINEL_T).all()
    ph.apply(ts, T_in=a, active=act)
    hist.record(a, ts, cc.DT, active=act)
    assert cc.same_bits(_host(hc, ts)[~act], np.full(shape, cc.SENTINEL_T)[~act])
    for t in (ph.f, hist.d_peak, hist.d_t_hi, hist.d_t_lo):
        assert cc.same_bits(_host(hc, t)[~act], np.full(shape, cc.SENTINEL_F)[~act])
    assert cc.same_bits(_host(hc, ts)[act], ref[0]['T'][act]) and cc.same_values(_host(hc, ph.f)[act], ref[0]['f'][act])


@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 1, 36)])
def test_a_cold_run_rewrites_no_zero(hc, shape):
    """nothing melts and nothing cools through a level: T and f hold +0.0 and -0.0 at rest, T_peak holds -0.0 under a +0.0
    field -- every bit pattern survives both passes"""
    import torch
    rng = np.random.default_rng(9)
    g = _grid(hc, shape)
    law, levels = cc.objects()
    T = rng.choice(np.array([0.0, -0.0, 300.0]), size=shape)
    f = rng.choice(np.array([0.0, -0.0]), size=shape)
    assert np.signbit(T).any() and np.signbit(f).any() and (~np.signbit(f)).any()
    ph = hc.CylPhaseField(g, hc.Material(*MAT), law)
    ph.f.copy_(_dev(g, f))
    hist = hc.CylThermalHistory(g, levels, capacity=2)
    peak = np.where(T == 0.0, -0.0, T)
    hist.d_peak.copy_(_dev(g, peak))
    a, ts = _dev(g, T), _dev(g, T)
    ph.apply(ts, T_in=a)
    hist.record(a, ts, 0.1)
    assert cc.same_bits(_host(hc, ts), T) and cc.same_bits(_host(hc, ph.f), f) and cc.same_bits(_host(hc, hist.d_peak), peak)
    assert np.isnan(_host(hc, hist.d_t_hi)).all() and np.isnan(_host(hc, hist.d_t_lo)).all()
    assert torch.equal(hist.d_log.cpu()[:cc.LOG_INTS], torch.from_numpy(cc.EMPTY_ROW))


def test_seed_kernels(hc):
    shape = (3, 5, 7)
    rng = np.random.default_rng(2)
    g = _grid(hc, shape)
    law, levels = cc.objects()
    T = rng.uniform(1300.0, 1500.0, shape)
    act = rng.random(shape) < 0.6
    sel = rng.random(shape) < 0.5
    ph = hc.CylPhaseField(g, hc.Material(*MAT), law, T=T, active=act)
    assert cc.same_values(_host(hc, ph.f), np.where(act, law.f_eq(T), np.nan))
    T2 = T + 40.0
    ph.seed(T2, sel=sel, active=act)
    assert cc.same_values(_host(hc, ph.f), np.where(act & sel, law.f_eq(T2), np.where(act, law.f_eq(T), np.nan)))
    hist = hc.CylThermalHistory(g, levels, capacity=1, T=T, active=act)
    assert cc.same_values(_host(hc, hist.d_peak), np.where(act, T, np.nan))
    hist.seed(T2, sel=sel, active=act)
    assert cc.same_values(_host(hc, hist.d_peak), np.where(act & sel, T2, np.where(act, T, np.nan)))
    snap = ph.snapshot(), hist.snapshot()
    ph.seed(T, active=None)
    hist.seed(T)
    ph.restore(snap[0])
    hist.restore(snap[1])
    assert cc.same_values(_host(hc, ph.f), np.where(act & sel, law.f_eq(T2), np.where(act, law.f_eq(T), np.nan)))
    assert cc.same_values(_host(hc, hist.d_peak), np.where(act & sel, T2, np.where(act, T, np.nan)))


# ---- the plain steps ---------------------------------------------------------------------------------------------------------
def _setup(hc, shape, r_in, zkinds=('neumann0', 'robin'), dt=0.05):
    g = _grid(hc, shape, r_in)
    mat, prm = hc.Material(*MAT), hc.Params(dt, 1.0, 'be')
    wall = hc.RobinR(25.0, 25.0)
    zbc = hc.ZBC(kind_bot=zkinds[0], kind_top=zkinds[1], h_top=15.0, T_inf_top=25.0, T_bot=1425.0, T_top=1380.0)
    return g, mat, prm, wall, zbc


@pytest.mark.parametrize('shape,r_in,zkinds', [((5, 8, 129), 0.03, ('neumann0', 'robin')), ((3, 5, 7), 0.0, ('dirichlet', 'robin')),
                                               ((2, 3, 1024), 0.0, ('neumann0', 'dirichlet'))])   # (a plan's longest line)
def test_step_keywords_are_the_plain_step_then_the_definitions(hc, shape, r_in, zkinds):
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField, CylThermalHistory
    g, mat, prm, wall, zbc = _setup(hc, shape, r_in, zkinds)
    law, levels = cc.objects()
    rng = np.random.default_rng(4)
    T = rng.uniform(1200.0, 1650.0, shape)
    act = rng.random(shape) < 0.7
    act[:, rng.random(shape[1:]) < 0.2] = False
    skip = CylPhaseField.skip_planes(shape, zkinds[0] == 'dirichlet', zkinds[1] == 'dirichlet')
    nan3 = tuple(np.full(shape, np.nan) for _ in range(3))
    # adi_step
    plain = np.asarray(hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc))
    assert cc.same_bits(plain, np.asarray(hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, phase=None, history=None)))
    ph = hc.CylPhaseField(g, mat, law, T=T)
    hist = hc.CylThermalHistory(g, levels, capacity=4, t=2.0)
    got = np.asarray(hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, phase=ph, history=hist))
    Tn, fn = CylPhaseField.apply_reference(plain, law.f_eq(T), T, None, skip, law, mat.cp)
    state, pool = CylThermalHistory.record_reference(nan3, T, Tn, None, 2.0, prm.dt, levels)
    assert not cc.same_bits(plain, Tn)
    assert cc.same_bits(got, Tn) and cc.same_values(_host(hc, ph.f), fn)
    for s, w in zip((hist.d_peak, hist.d_t_hi, hist.d_t_lo), state):
        assert cc.same_values(_host(hc, s), w)
    assert np.array_equal(_log(hist)[1][0], CylThermalHistory.pool_row(pool)) and hist.slot == 1 and hist.t == 2.0 + prm.dt
    # adi_step_masked: the same objects see `act` for the first time on some cells that are already seeded, and that is fine
    Tm = np.where(act, T, 25.0)
    plain = np.asarray(hc.adi_step_masked(hc.to_device(Tm), g, mat, prm, wall, zbc, act))
    assert cc.same_bits(plain, np.asarray(hc.adi_step_masked(hc.to_device(Tm), g, mat, prm, wall, zbc, act, phase=None,
                                                             history=None)))
    ph = hc.CylPhaseField(g, mat, law, active=np.zeros(shape, bool))
    hist = hc.CylThermalHistory(g, levels, capacity=4, t=0.25)
    got = np.asarray(hc.adi_step_masked(hc.to_device(Tm), g, mat, prm, wall, zbc, act, phase=ph, history=hist))
    Tn, fn = CylPhaseField.apply_reference(plain, np.full(shape, np.nan), Tm, act, skip, law, mat.cp)
    state, pool = CylThermalHistory.record_reference(nan3, Tm, Tn, act, 0.25, prm.dt, levels)
    assert cc.same_bits(got, Tn) and cc.same_values(_host(hc, ph.f), fn)
    for s, w in zip((hist.d_peak, hist.d_t_hi, hist.d_t_lo), state):
        assert cc.same_values(_host(hc, s), w)
    assert np.array_equal(_log(hist)[1][0], CylThermalHistory.pool_row(pool))
    # errors before the first launch
    other = _grid(hc, shape, r_in)
    with pytest.raises(ValueError, match='another grid'):
        hc.adi_step(hc.to_device(T), other, mat, prm, wall, zbc, phase=ph)
    with pytest.raises(TypeError):
        hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, history=ph)
    assert hist.slot == 1


# ---- the stepper -----------------------------------------------------------------------------------------------------------------
def _stepper_state(hc, ph, hist):
    out = []
    if ph is not None:
        out.append(_host(hc, ph.f))
    if hist is not None:
        out += [_host(hc, s) for s in (hist.d_peak, hist.d_t_hi, hist.d_t_lo)]
        # the clock: a run leaves the block at (t0, n), single steps at (t0 + (n - 1) dt, 1) -- the time t0 + n dt is what both
        # must agree on, with the slot and the capacity
        blk = hist.d_block.cpu().numpy()
        t0, dt = blk.view(np.float64)[:2]
        out += [hist._log_store.cpu().numpy().astype(np.float64), np.array([t0 + blk[2] * dt, dt, blk[3], blk[4]]),
                np.array([hist.slot, hist.t] + list(hist._times))]
    return out


@pytest.mark.parametrize('with_history', [True, False], ids=['phase+history', 'phase'])
@pytest.mark.parametrize('shape,zkinds', [((5, 8, 129), ('neumann0', 'robin')), ((2, 1, 36), ('dirichlet', 'robin'))])
def test_stepper_run_is_step_called_n_times(hc, shape, zkinds, with_history):
    g, mat, prm, wall, zbc = _setup(hc, shape, 0.03, zkinds, dt=0.0625)      # (a dt whose multiples from t = 1 are exact: the
    law, levels = cc.objects()                                               # clocks of run and of step() then agree to the bit)
    rng = np.random.default_rng(6)
    T = rng.uniform(1200.0, 1650.0, shape)

    def fresh():
        ph = hc.CylPhaseField(g, mat, law, T=T)
        hist = hc.CylThermalHistory(g, levels, capacity=8, t=1.0) if with_history else None
        return ph, hist, hc.StagedCylStepper(g, mat, prm, wall, zbc, phase=ph, history=hist)

    def by_steps(st, ph, hist, T, n):
        cur = hc.to_device(T)
        for _ in range(n):
            cur = st.step(cur)
        return [np.asarray(cur)] + _stepper_state(hc, ph, hist)

    for graph in (True, False):
        for n in (1, 2, 5):
            ph_r, hist_r, st_r = fresh()
            ph_s, hist_s, st_s = fresh()
            want = by_steps(st_s, ph_s, hist_s, T, n)
            got = [np.asarray(st_r.run(hc.to_device(T), n, graph=graph))] + _stepper_state(hc, ph_r, hist_r)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert cc.same_values(a, b), (graph, n)
            assert cc.same_bits(got[0], want[0])
            assert st_r.captures == (1 if graph and n >= 2 else 0)
        # a second run of the objects that did 5 steps, on the same graph, from another field and another t0
        T2 = want[0] * 0.98
        want = by_steps(st_s, ph_s, hist_s, T2, 3)
        got = [np.asarray(st_r.run(hc.to_device(T2), 3, graph=graph, t0=7.5))] + _stepper_state(hc, ph_r, hist_r)
        for a, b in zip(got, want):
            assert cc.same_values(a, b), graph
        assert cc.same_bits(got[0], want[0])
        assert st_r.captures == (1 if graph else 0)
    if with_history:
        assert hist_r.slot == 8 and np.isfinite(_host(hc, hist_r.d_peak)).all()
    assert ((want[1] > 0.0) & (want[1] < 1.0)).any()                       # (f: the run sits in the mushy range)
    with pytest.raises(TypeError):
        hc.StagedCylStepper(g, mat, prm, wall, zbc, phase=levels)
    with pytest.raises(ValueError, match='another grid'):
        hc.StagedCylStepper(_grid(hc, shape, 0.03), mat, prm, wall, zbc, history=hc.CylThermalHistory(g, levels, capacity=1))


def test_stepper_without_keywords_is_unchanged(hc):
    shape = (5, 8, 129)
    g, mat, prm, wall, zbc = _setup(hc, shape, 0.03)
    T = np.random.default_rng(8).uniform(300.0, 1650.0, shape)
    st = hc.StagedCylStepper(g, mat, prm, wall, zbc)
    cur = hc.to_device(T)
    for _ in range(3):
        cur = hc.adi_step(cur, g, mat, prm, wall, zbc)
    assert cc.same_bits(np.asarray(st.run(hc.to_device(T), 3)), np.asarray(cur))
    assert cc.same_bits(np.asarray(st.run(hc.to_device(T), 3, graph=False)), np.asarray(cur))
    assert st.captures == 1 and st._graph['Y'] is None


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_spiral_deposition_with_latent_heat_and_history(hc):
    from adi_thermal_fields_amd import waam
    from adi_thermal_fields_amd.phase import PhaseChange
    from adi_thermal_fields_amd.history import HistoryLevels
    law, levels = PhaseChange(*cc.SPIRAL_LAW), HistoryLevels(*cc.SPIRAL_LEVELS)
    ref = cc.spiral_reference(law, levels)
    assert ref['margin'] > 1e-6                                   # first: no comparison of the reference sits on a level
    grid, fields, masks, f, hist = waam.run_spiral_deposition(hc, *cc.spiral_args(), phase_change=law, history=levels)
    _, plain, pmasks = waam.run_spiral_deposition(hc, *cc.spiral_args())
    Tmax = max(float(np.max(np.abs(a))) for a in ref['fields'])
    Ts, Tl = cc.SPIRAL_LAW[1:]
    for a, b, ma, mb in zip(fields, ref['fields'], masks, ref['masks']):
        assert np.array_equal(ma, mb)
        assert float(np.max(np.abs(a - b))) / float(np.max(np.abs(b))) <= 1e-10
    assert any(float(np.max(np.abs(a - b))) > 1.0 for a, b in zip(fields, plain))        # (the latent heat is felt)
    act = ref['masks'][-1]
    assert np.array_equal(np.isnan(ref['f']), ~act) and (f[~act] == 0.0).all()
    assert float(np.max(np.abs(f[act] - ref['f'][act]))) <= 1e-10 * Tmax / (Tl - Ts)
    peak = ref['state'][0]
    assert np.array_equal(np.isnan(hist['T_peak']), np.isnan(peak)) and np.array_equal(np.isnan(peak), ~act)
    assert float(np.nanmax(np.abs(hist['T_peak'] - peak))) / float(np.nanmax(np.abs(peak))) <= 1e-10
    for key, want, slope in (('t_hi', ref['state'][1], ref['slope_hi']), ('t_lo', ref['state'][2], ref['slope_lo'])):
        assert np.array_equal(np.isnan(hist[key]), np.isnan(want)), key
        on = np.isfinite(want)
        assert on.any() and np.isfinite(slope[on]).all()
        # an error of 1e-10 max|T| in A or B moves the crossing by that times dt / (A - B) of the cell; the clocks add rounding
        tol = 1e-10 * Tmax * slope[on] + 8 * np.finfo(np.float64).eps * np.abs(want[on])
        assert (np.abs(hist[key][on] - want[on]) <= tol).all(), key
    with np.errstate(invalid='ignore'):
        assert cc.same_values(hist['cooling_time'], hist['t_lo'] - hist['t_hi'])
    pool = hist['melt_pool']
    rows = np.array(ref['rows'])
    assert pool['dropped'] == 0 and len(pool['cells']) == len(rows) == 40
    assert np.array_equal(pool['cells'], rows[:, 0]) and np.array_equal(pool['lo'], rows[:, 1:4])
    assert np.array_equal(pool['hi'], rows[:, 4:7])
    assert np.array_equal(pool['sum_i'], np.ascontiguousarray(rows[:, 8:10]).view(np.int64)[:, 0])
    assert np.allclose(pool['t'], ref['t_end'], rtol=0, atol=1e-12) and pool['cells'].max() > 0
    with pytest.raises(ValueError, match='needs the device loop'):
        waam.run_spiral_deposition(hc, *cc.spiral_args(), history=levels, device_resident=False)
