"""GPU: the cylindrical field monitor -- adi_cyl_monitor_record against the NumPy definition and its host twin, bit for bit, on
every case of cyl_monitor_cases.py; the guard words and the spill row; the keyword of adi_step / adi_step_masked;
StagedCylStepper.run against step(); run_spiral_deposition against the oracle's loop followed by the definition."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cyl_monitor_cases as mc  # noqa: E402
import cyl_extras_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = mc.case_ids()
MAT = (7800.0, cc.CP, 30.0)


@pytest.fixture(scope='module')
def hc():
    import torch
    assert torch.cuda.is_available()
    import adi_thermal_fields_amd.adi3d_hip_cyl as hipcyl
    return hipcyl


def _grid(hc, shape, r_in=0.0, dr=mc.DR, dz=1.2e-3):
    nr, nphi, nz = shape
    return hc.GridCyl(nr, nphi, nz, dr, 2.0 * math.pi / nphi, dz, r_in + nr * dr, R_in=r_in)


def _dev(g, a):
    import torch
    return g.layout.to_layout(np.ascontiguousarray(a), torch.float64)


def _host(hc, t):
    return np.asarray(hc.DeviceField(t))


def _guards_ok(mon):
    lo, hi = mon.guards()
    return (lo == mc.GUARD_WORD).all() and (hi == mc.GUARD_WORD).all() and len(lo) == mc.GUARD


@pytest.mark.parametrize('c', CASES, ids=mc.case_name)
def test_device_row_is_the_definition_and_the_host_twin_bit_for_bit(hc, c):
    """with `extra` (NaN cells included) on the first two records' shapes and modes alike; the third record re-reads the same
    buffers, so a stale partial would show"""
    shape, mode, r_in = c
    case, refs = mc.reference(shape, mode, r_in)
    _, host_rows, _ = mc.host_rows(case, r_in)
    g = _grid(hc, shape, r_in)
    extra = g.layout.empty()
    mon = hc.CylFieldMonitor(g, probes=case['probes'], regions=case['regions'], capacity=mc.NREC, extra=extra, t=mc.T0_CLOCK)
    for n in range(mc.NREC):
        extra.copy_(_dev(g, case['extras'][n]))
        mon.record(_dev(g, case['fields'][n]), mc.DT, active=case['acts'][n])
    rows, dropped = mon.rows()
    assert dropped == 0 and mon.slot == mc.NREC and mon.t == mc.T0_CLOCK + mc.NREC * mc.DT
    assert mc.same_rows(rows, mc.reference_rows(refs))
    assert mc.same_rows(rows, host_rows[:mc.NREC])
    npr = len(case['probes'])
    assert np.array_equal(rows[:, npr::mc.REGION_WORDS], np.array([r['cells'] for r in refs]))
    assert np.array_equal(rows[:, npr + 1::mc.REGION_WORDS], np.array([r['sum_i'] for r in refs]))
    assert _guards_ok(mon)
    assert np.isnan(mon.d_log.cpu().numpy().view(np.float64)[-mon.row_words:]).all()      # the spill row: untouched
    tr = mon.traces()
    assert mc.same_rows(tr['T'].T.copy().view(np.int64), np.array([r['probes'] for r in refs]).view(np.int64))
    assert list(tr['t']) == [mc.T0_CLOCK + (n + 1) * mc.DT for n in range(mc.NREC)]


@pytest.mark.parametrize('c', CASES[::3] + CASES[2::3], ids=mc.case_name)
def test_device_row_without_extra(hc, c):
    shape, mode, r_in = c
    case, refs = mc.reference(shape, mode, r_in, False)
    g = _grid(hc, shape, r_in)
    mon = hc.CylFieldMonitor(g, probes=case['probes'], regions=case['regions'], capacity=mc.NREC)
    for n in range(mc.NREC):
        mon.record(_dev(g, case['fields'][n]), 0.0, active=case['acts'][n])
    rows, _ = mon.rows()
    assert mc.same_rows(rows, mc.reference_rows(refs)) and _guards_ok(mon) and mon.t == 0.0
    log = mon.region_log(hc.Material(*MAT))
    assert 'extra_volume' not in log and np.array_equal(log['cells'].T, np.array([r['cells'] for r in refs]))
    from adi_thermal_fields_amd.cyl_extras import CylThermalHistory
    assert mc.same_rows(log['volume'].view(np.int64), CylThermalHistory.pool_volume(g, log['cells'], log['sum_i']).view(np.int64))
    assert mc.same_rows(log['heat'].view(np.int64), ((MAT[0] * MAT[1]) * (g.dr * g.dphi * g.dz) * log['sum_rT']).view(np.int64))


def test_capacity_2_spill_row_dropped_reset_and_snapshot(hc):
    shape, r_in = (5, 8, 129), 0.03
    case, refs = mc.reference(shape, 'births', r_in)
    want = mc.reference_rows(refs)
    g = _grid(hc, shape, r_in)
    extra = _dev(g, case['extras'][0])
    mon = hc.CylFieldMonitor(g, probes=case['probes'], regions=case['regions'], capacity=2, extra=extra)
    order = (0, 1, 2, 0, 1)
    for n in order:
        extra.copy_(_dev(g, case['extras'][n]))
        mon.record(_dev(g, case['fields'][n]), mc.DT, active=case['acts'][n])
        if mon.slot == 2:
            snap = mon.snapshot()
    rows, dropped = mon.rows()
    assert dropped == 3 and mon.slot == 5 and mc.same_rows(rows, want[:2])
    spill = mon.d_log.cpu().numpy()[-mon.row_words:]
    assert mc.same_rows(spill, want[1]) and _guards_ok(mon)             # the spill row holds the last record
    assert mon.region_log()['dropped'] == 3 and mon.region_log()['cells'].shape[1] == 2
    mon.restore(snap)
    assert mon.slot == 2 and mon.t == 2 * mc.DT and np.isnan(mon.d_log.cpu().numpy().view(np.float64)[-mon.row_words:]).all()
    mon.reset(t=0.5)
    assert mon.slot == 0 and mon.t == 0.5 and np.isnan(mon.d_log.cpu().numpy().view(np.float64)).all() and _guards_ok(mon)
    assert mon.rows()[0].shape == (0, mon.row_words)


def test_constructor_errors(hc):
    g = _grid(hc, (3, 5, 7))
    with pytest.raises(ValueError):
        hc.CylFieldMonitor(g, regions=[((0, 3), (5, 6), (0, 7))])
    with pytest.raises(ValueError):
        hc.CylFieldMonitor(g, probes=[(3, 0, 0)])
    with pytest.raises(ValueError):
        hc.CylFieldMonitor(g, capacity=0)
    with pytest.raises((ValueError, TypeError)):
        hc.CylFieldMonitor(g, extra=np.zeros((3, 5, 7)))
    mon = hc.CylFieldMonitor(g)
    with pytest.raises(ValueError):
        mon.record(g.layout.empty(zero=True), -1.0)
    assert mon.slot == 0 and mon.regions == (((0, 3), (0, 5), (0, 7)),)


# ---- the plain steps ---------------------------------------------------------------------------------------------------------
def _setup(hc, shape, r_in, zkinds=('neumann0', 'robin'), dt=0.05):
    g = _grid(hc, shape, r_in)
    mat, prm = hc.Material(*MAT), hc.Params(dt, 1.0, 'be')
    wall = hc.RobinR(25.0, 25.0)
    zbc = hc.ZBC(kind_bot=zkinds[0], kind_top=zkinds[1], h_top=15.0, T_inf_top=25.0, T_bot=1425.0, T_top=1380.0)
    return g, mat, prm, wall, zbc


def _regions(shape):
    nr, nphi, nz = shape
    return [None, ((0, nr), (nphi - 1, nphi + 1) if nphi > 1 else (0, 1), (1, nz - 1))]


@pytest.mark.parametrize('shape,r_in', [((5, 8, 129), 0.03), ((3, 5, 7), 0.0), ((2, 3, 1024), 0.0)])   # (a plan's longest line)
def test_step_keyword_is_the_plain_step_then_the_definition(hc, shape, r_in):
    from adi_thermal_fields_amd.cyl_monitor import CylFieldMonitor
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField
    g, mat, prm, wall, zbc = _setup(hc, shape, r_in)
    law, levels = cc.objects()
    rng = np.random.default_rng(4)
    T = rng.uniform(1200.0, 1650.0, shape)
    act = rng.random(shape) < 0.7
    act[:, rng.random(shape[1:]) < 0.2] = False
    probes, regions = [(0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1)], _regions(shape)
    # adi_step, the monitor alone
    plain = np.asarray(hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc))
    mon = hc.CylFieldMonitor(g, probes=probes, regions=regions, capacity=4, t=2.0)
    got = np.asarray(hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, monitor=mon))
    assert cc.same_bits(got, plain)
    want = CylFieldMonitor.row_of(CylFieldMonitor.record_reference(plain, None, probes, regions, g))
    assert mc.same_rows(mon.rows()[0], want[None]) and mon.slot == 1 and mon.t == 2.0 + prm.dt
    # adi_step_masked next to phase= and history=, extra = ph.f
    Tm = np.where(act, T, 25.0)
    ph0 = hc.CylPhaseField(g, mat, law, active=np.zeros(shape, bool))
    hist0 = hc.CylThermalHistory(g, levels, capacity=4, t=0.25)
    base = np.asarray(hc.adi_step_masked(hc.to_device(Tm), g, mat, prm, wall, zbc, act, phase=ph0, history=hist0))
    ph = hc.CylPhaseField(g, mat, law, active=np.zeros(shape, bool))
    hist = hc.CylThermalHistory(g, levels, capacity=4, t=0.25)
    mon = hc.CylFieldMonitor(g, probes=probes, regions=regions, capacity=4, extra=ph.f, t=0.25)
    got = np.asarray(hc.adi_step_masked(hc.to_device(Tm), g, mat, prm, wall, zbc, act, phase=ph, history=hist, monitor=mon))
    assert cc.same_bits(got, base) and cc.same_values(_host(hc, ph.f), _host(hc, ph0.f))
    assert np.array_equal(hist._log_store.cpu().numpy(), hist0._log_store.cpu().numpy())
    f = _host(hc, ph.f)
    assert np.isnan(f[~act]).all() and ((f[act] > 0.0) & (f[act] < 1.0)).any()
    want = CylFieldMonitor.row_of(CylFieldMonitor.record_reference(base, act, probes, regions, g, extra=f))
    assert mc.same_rows(mon.rows()[0], want[None]) and mon.t == 0.25 + prm.dt
    log = mon.region_log(mat)
    assert log['extra_volume'][0, 0] > 0.0 and log['cells'][0, 0] == act.sum()
    # adi_step with all three
    ph = hc.CylPhaseField(g, mat, law, T=T)
    skip = CylPhaseField.skip_planes(shape)
    Tn, fn = CylPhaseField.apply_reference(plain, law.f_eq(T), T, None, skip, law, mat.cp)
    mon = hc.CylFieldMonitor(g, regions=regions, capacity=1, extra=ph.f)
    got = np.asarray(hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, phase=ph,
                                 history=hc.CylThermalHistory(g, levels, capacity=1), monitor=mon))
    assert cc.same_bits(got, Tn)
    want = CylFieldMonitor.row_of(CylFieldMonitor.record_reference(Tn, None, (), regions, g, extra=fn))
    assert mc.same_rows(mon.rows()[0], want[None])
    # errors before the first launch
    with pytest.raises(ValueError, match='another grid'):
        hc.adi_step(hc.to_device(T), _grid(hc, shape, r_in), mat, prm, wall, zbc, monitor=mon)
    with pytest.raises(TypeError):
        hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, monitor=ph)
    from adi_thermal_fields_amd.monitor import FieldMonitor
    with pytest.raises(TypeError):                                  # a Cartesian monitor is another type (no instance needed:
        hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, monitor=FieldMonitor.__new__(FieldMonitor))   # the check is first)
    assert mon.slot == 1


# ---- the stepper -----------------------------------------------------------------------------------------------------------------
def _state(hc, ph, hist, mon):
    out = []
    if ph is not None:
        out.append(_host(hc, ph.f))
    for rec in (hist, mon):
        if rec is None:
            continue
        # the clock: a run leaves the block at (t0, n), single steps at (t0 + (n - 1) dt, 1) -- the time t0 + n dt is what both
        # must agree on, with the slot and the capacity
        blk = rec.d_block.cpu().numpy()
        t0, dt = blk.view(np.float64)[:2]
        out += [np.array([rec.slot, rec.t] + list(rec._times))]
        if rec is hist:
            out += [_host(hc, s) for s in (hist.d_peak, hist.d_t_hi, hist.d_t_lo)]
            out += [hist._log_store.cpu().numpy().astype(np.float64), np.array([t0 + blk[2] * dt, dt, blk[3], blk[4]])]
        else:
            out += [mon._log_store.cpu().numpy().view(np.float64), np.array([blk[3], blk[4]])]   # (the monitor reads no time)
    return out


@pytest.mark.parametrize('extras', ['monitor', 'phase+monitor', 'phase+history+monitor', 'history+monitor'])
@pytest.mark.parametrize('shape,zkinds', [((5, 8, 129), ('neumann0', 'robin')), ((2, 1, 36), ('dirichlet', 'robin'))])
def test_stepper_run_is_step_called_n_times(hc, shape, zkinds, extras):
    from adi_thermal_fields_amd.cyl_monitor import CylFieldMonitor
    g, mat, prm, wall, zbc = _setup(hc, shape, 0.03, zkinds, dt=0.0625)      # (a dt whose multiples from t = 1 are exact: the
    law, levels = cc.objects()                                               # clocks of run and of step() then agree to the bit)
    rng = np.random.default_rng(6)
    T = rng.uniform(1200.0, 1650.0, shape)
    probes, regions = [(0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1)], _regions(shape)

    def fresh():
        ph = hc.CylPhaseField(g, mat, law, T=T) if 'phase' in extras else None
        hist = hc.CylThermalHistory(g, levels, capacity=8, t=1.0) if 'history' in extras else None
        mon = hc.CylFieldMonitor(g, probes=probes, regions=regions, capacity=8, extra=None if ph is None else ph.f, t=1.0)
        return ph, hist, mon, hc.StagedCylStepper(g, mat, prm, wall, zbc, phase=ph, history=hist, monitor=mon)

    def by_steps(st, objs, T, n):
        cur = hc.to_device(T)
        fields = []
        for _ in range(n):
            cur = st.step(cur)
            fields.append((np.asarray(cur), None if objs[0] is None else _host(hc, objs[0].f)))
        return [np.asarray(cur)] + _state(hc, *objs), fields

    for graph in (True, False):
        for n in (1, 2, 5):
            *objs_r, st_r = fresh()
            *objs_s, st_s = fresh()
            want, fields = by_steps(st_s, objs_s, T, n)
            got = [np.asarray(st_r.run(hc.to_device(T), n, graph=graph))] + _state(hc, *objs_r)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert cc.same_values(a, b), (graph, n)
            assert cc.same_bits(got[0], want[0])
            assert st_r.captures == (1 if graph and n >= 2 else 0)
            if 'history' not in extras:
                assert st_r._graph['Y'] is None
            # the rows are the definition of every step's final field
            rows, dropped = objs_r[2].rows()
            assert dropped == 0 and len(rows) == n
            for k, (Tk, fk) in enumerate(fields):
                ref = CylFieldMonitor.record_reference(Tk, None, probes, regions, g, extra=fk)
                assert mc.same_rows(rows[k], CylFieldMonitor.row_of(ref)), (graph, n, k)
        # a second run of the objects that did 5 steps, on the same graph, from another field and another t0
        T2 = want[0] * 0.98
        want, _ = by_steps(st_s, objs_s, T2, 3)
        got = [np.asarray(st_r.run(hc.to_device(T2), 3, graph=graph, t0=7.5))] + _state(hc, *objs_r)
        for a, b in zip(got, want):
            assert cc.same_values(a, b), graph
        assert cc.same_bits(got[0], want[0])
        assert st_r.captures == (1 if graph else 0)
        assert objs_r[2].slot == 8 and objs_r[2].t == 1.0 + 8 * 0.0625
    with pytest.raises(TypeError):
        hc.StagedCylStepper(g, mat, prm, wall, zbc, monitor=levels)
    with pytest.raises(ValueError, match='another grid'):
        hc.StagedCylStepper(_grid(hc, shape, 0.03), mat, prm, wall, zbc, monitor=hc.CylFieldMonitor(g))


def test_stepper_without_the_keyword_is_unchanged(hc):
    shape = (5, 8, 129)
    g, mat, prm, wall, zbc = _setup(hc, shape, 0.03)
    T = np.random.default_rng(8).uniform(300.0, 1650.0, shape)
    st = hc.StagedCylStepper(g, mat, prm, wall, zbc, monitor=None)
    cur = hc.to_device(T)
    for _ in range(3):
        cur = hc.adi_step(cur, g, mat, prm, wall, zbc, monitor=None)
    assert cc.same_bits(np.asarray(st.run(hc.to_device(T), 3)), np.asarray(cur))
    assert cc.same_bits(np.asarray(st.run(hc.to_device(T), 3, graph=False)), np.asarray(cur))
    assert st.captures == 1 and st._graph['Y'] is None and st._graph['key'] == (None, None, None)
    # a monitor joins the key: another monitor is another graph
    mon_a, mon_b = hc.CylFieldMonitor(g), hc.CylFieldMonitor(g)
    st = hc.StagedCylStepper(g, mat, prm, wall, zbc, monitor=mon_a)
    assert cc.same_bits(np.asarray(st.run(hc.to_device(T), 3)), np.asarray(cur)) and st.captures == 1
    st.monitor = mon_b
    assert cc.same_bits(np.asarray(st.run(hc.to_device(T), 3)), np.asarray(cur)) and st.captures == 2
    assert mon_a.slot == 3 and mon_b.slot == 3 and mc.same_rows(mon_a.rows()[0], mon_b.rows()[0])


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_spiral_deposition_with_a_monitor(hc):
    """against the oracle's adi_step_masked loop (cyl_extras_cases.spiral_reference, with latent heat) followed by the
    definition on each step's reference field: probes to 1e-10 of max|T|, sums to 1e-10 of sum|terms|, integers equal"""
    from adi_thermal_fields_amd import waam
    from adi_thermal_fields_amd.cyl_monitor import CylFieldMonitor
    from adi_thermal_fields_amd.phase import PhaseChange
    from adi_thermal_fields_amd.history import HistoryLevels
    s = cc.SPIRAL
    law, levels = PhaseChange(*cc.SPIRAL_LAW), HistoryLevels(*cc.SPIRAL_LEVELS)
    nr, nphi = s['nr'], s['nphi']
    nz = int(round((s['z_back'] + s['layer_h'] * s['n_layers']) / s['layer_h']))
    probes = [(0, 0, nz - 1), (nr - 1, nphi - 1, nz - 2), (1, 3, 0)]
    regions = [None, ((0, nr), (nphi - 2, nphi + 3), (nz - 2, nz)), ((1, 3), (2, 6), (0, nz))]
    # the reference: spiral_reference's loop, keeping every step's field, mask and f
    steps = []
    ref = _spiral_steps(cc, law, levels, steps)
    assert len(steps) == 40
    grid, fields, masks, f, traces, log = waam.run_spiral_deposition(hc, *cc.spiral_args(), phase_change=law,
                                                                     monitor=dict(probes=probes, regions=regions, extra_f=True))
    for a, b in zip(fields, ref['fields']):
        assert float(np.max(np.abs(a - b))) / float(np.max(np.abs(b))) <= 1e-10
    assert traces['T'].shape == (3, 40) and log['cells'].shape == (3, 40) and log['dropped'] == 0
    assert np.allclose(traces['t'], ref['t_end'], rtol=0, atol=1e-12)
    Tmax = max(float(np.max(np.abs(a))) for a in ref['fields'])
    r = np.asarray(grid.r)[:, None, None]
    boxes = CylFieldMonitor.checked_regions(grid.shape, regions)
    seen_nan = seen_val = False
    for n, (Tn, act, fn) in enumerate(steps):
        want = CylFieldMonitor.record_reference(Tn, act, probes, regions, grid, extra=fn)
        assert np.array_equal(log['cells'][:, n], want['cells']) and np.array_equal(log['sum_i'][:, n], want['sum_i'])
        assert np.array_equal(np.isnan(traces['T'][:, n]), np.isnan(want['probes']))
        on = ~np.isnan(want['probes'])
        seen_nan, seen_val = seen_nan or (~on).any(), seen_val or on.any()
        assert (np.abs(traces['T'][on, n] - want['probes'][on]) <= 1e-10 * Tmax).all()
        X = np.nan_to_num(fn, nan=0.0)
        for q, box in enumerate(boxes):
            inc = CylFieldMonitor.region_cells(grid.shape, box) & act
            for key, terms in (('sum_T', Tn[inc]), ('sum_rT', (r * Tn)[inc]), ('sum_extra', X[inc]), ('sum_rextra', (r * X)[inc])):
                assert abs(log[key][q, n] - want[key][q]) <= 1e-10 * float(np.sum(np.abs(terms))), (n, q, key)
            for key in ('T_min', 'T_max'):
                assert abs(log[key][q, n] - want[key][q]) <= 1e-10 * Tmax
    assert seen_nan and seen_val and log['extra_volume'].max() > 0.0 and 'heat' in log
    with pytest.raises(ValueError, match='needs the device loop'):
        waam.run_spiral_deposition(hc, *cc.spiral_args(), monitor=dict(probes=probes), device_resident=False)
    with pytest.raises(ValueError, match='needs phase_change'):
        waam.run_spiral_deposition(hc, *cc.spiral_args(), monitor=dict(extra_f=True))


def _spiral_steps(cc, law, levels, steps):
    """cyl_extras_cases.spiral_reference, with every step's (final field, mask, f) appended to `steps`: the loop calls the
    definition CylPhaseField.apply_reference once per step, which is where the three are taken"""
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField
    orig = CylPhaseField.apply_reference

    def keeping(T_star, f, T_in, active, skip, law_, cp):
        Tn, fn = orig(T_star, f, T_in, active, skip, law_, cp)
        steps.append((Tn.copy(), np.array(active, dtype=bool), fn.copy()))
        return Tn, fn
    CylPhaseField.apply_reference = staticmethod(keeping)
    try:
        return cc.spiral_reference(law, levels)
    finally:
        CylPhaseField.apply_reference = staticmethod(orig)
