"""GPU: the solidification record of the cylindrical step -- the kernel adi_cyl_solid_record against the NumPy definition and its
host twin, bit for bit, on every case of cyl_solid_cases.py; what it must never write; the hot words; the keyword of adi_step /
adi_step_masked; StagedCylStepper.run against step(); run_spiral_deposition against the reference loop (the oracle's
adi_step_masked, CylPhaseField.apply_reference, then the definition)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cyl_extras_cases as cc  # noqa: E402
import cyl_solid_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sc.case_ids()
MAT = (7800.0, cc.CP, 30.0)
EPS = np.finfo(np.float64).eps


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


def _state(hc, rec):
    return tuple(_host(hc, s) for s in (rec.d_t_solid, rec.d_rate, rec.d_g2))


def _log(rec):
    n = sc.LOG_INTS
    store = rec._log_store.cpu().numpy()
    return store, store[sc.GUARD:sc.GUARD + (rec.capacity + 1) * n].reshape(rec.capacity + 1, n)


def _guards_intact(rec):
    log, hot = rec._log_store.cpu().numpy(), rec._hot_store.cpu().numpy()
    return all((a[:sc.GUARD] == sc.GUARD_WORD).all() and (a[-sc.GUARD:] == sc.GUARD_WORD).all() for a in (log, hot))


@pytest.fixture(scope='module')
def loops():
    """the reference loop and the host-twin loop of every case, computed once"""
    out = {}
    for shape, mode, r_in in CASES:
        case = sc.make_case(shape, mode)
        grid = sc.Grid(shape, r_in)
        out[(shape, mode)] = (sc.reference_loop(case, grid), sc.host_loop(case, grid))
    return out


@pytest.mark.parametrize('c', CASES, ids=sc.case_name)
def test_kernel_is_the_definition_and_the_host_twin_bit_for_bit(hc, loops, c):
    shape, mode, r_in = c
    (ref, ref_log), (host, _, host_rows, _) = loops[(shape, mode)]
    g = _grid(hc, shape, r_in)
    rec = hc.CylSolidificationRecord(g, sc.T_F, capacity=sc.NSTEPS, t=sc.T0_CLOCK)
    for n, r in enumerate(ref):
        rec.record(_dev(g, r['A']), _dev(g, r['B']), sc.DT, active=r['act'])
        got = _state(hc, rec)
        for want in (r['state'], host[n]['state']):
            for a, b in zip(got, want):
                assert sc.same_values(a, b), n
    store, rows = _log(rec)
    assert np.array_equal(rows, ref_log) and np.array_equal(rows, host_rows) and _guards_intact(rec)
    assert rec.slot == sc.NSTEPS and rec.t == sc.T0_CLOCK + sc.NSTEPS * sc.DT
    front = rec.front()
    assert np.array_equal(front['cells'], ref_log[:sc.NSTEPS, 0]) and front['dropped'] == 0 and front['cells'].max() > 0
    for n, r in enumerate(ref):
        act = np.ones(shape, bool) if r['act'] is None else r['act']
        cells = act & (r['A'] > sc.T_F) & (r['B'] <= sc.T_F)
        want = float(np.sum(np.broadcast_to(g.r[:, None, None], shape)[cells].astype(np.longdouble) * np.longdouble(g.dr)
                            * np.longdouble(g.dphi) * np.longdouble(g.dz)))
        assert abs(front['volume'][n] - want) <= 4 * EPS * want
        assert front['t'][n] == sc.T0_CLOCK + (n + 1) * sc.DT
        assert np.array_equal(front['lo'][n], r['front']['lo']) and np.array_equal(front['hi'][n], r['front']['hi'])
    with np.errstate(invalid='ignore', divide='ignore'):
        assert sc.same_values(np.asarray(rec.G), np.sqrt(ref[-1]['state'][2]))
        assert sc.same_values(np.asarray(rec.R), ref[-1]['state'][1] / np.sqrt(ref[-1]['state'][2]))
    snap = rec.snapshot()
    rec.reset(t=0.5)
    assert rec.slot == 0 and rec.t == 0.5 and all(np.isnan(s).all() for s in _state(hc, rec))
    assert np.array_equal(_log(rec)[1], np.tile(sc.EMPTY_ROW, (sc.NSTEPS + 1, 1))) and len(rec.front()['cells']) == 0
    rec.restore(snap)
    assert rec.slot == sc.NSTEPS and np.array_equal(_log(rec)[1], ref_log)
    for a, b in zip(_state(hc, rec), ref[-1]['state']):
        assert sc.same_values(a, b)


@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 3, 1030)])
def test_sentinels_keep_every_bit_outside_the_freezing_cells(hc, shape):
    case = sc.make_case(shape, 'random', seed=5)
    A, B, act = sc.chain(case)[0]
    g = _grid(hc, shape, 0.03)
    Rec = hc.CylSolidificationRecord
    rec = Rec(g, sc.T_F, capacity=2)
    for t in (rec.d_t_solid, rec.d_rate, rec.d_g2):
        t.fill_(sc.SENTINEL)
    rec.record(_dev(g, A), _dev(g, B), sc.DT, active=act)
    fz = act & (A > sc.T_F) & (B <= sc.T_F)
    want, _ = Rec.record_reference(sc.nan_state(shape), A, B, act, 0.0, sc.DT, sc.Grid(shape, 0.03), sc.T_F)
    assert fz.any() and (~fz & act).any()
    for got, w in zip(_state(hc, rec), want):
        assert sc.same_bits(got[~fz], np.full(shape, sc.SENTINEL)[~fz])
        assert sc.same_values(got[fz], w[fz])


@pytest.mark.parametrize('hot', [False, True], ids=['null', 'hot'])
@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 1, 36), (2, 3, 1030)])
def test_a_run_in_which_nothing_freezes_writes_nothing(hc, shape, hot):
    rng = np.random.default_rng(9)
    g = _grid(hc, shape)
    A = rng.uniform(300.0, 900.0, shape)
    A[0, 0, :3] = (1500.0, 1425.0, 1424.0)              # stays above; sits on the level; below: none of them freezes
    B = A - 10.0
    B[0, 0, 0] = 1430.0
    rec = hc.CylSolidificationRecord(g, sc.T_F, capacity=2)
    for t in (rec.d_t_solid, rec.d_rate, rec.d_g2):
        t.fill_(sc.SENTINEL)
    if hot:
        rec.seed_hot(_dev(g, A))
    rec.record(_dev(g, A), _dev(g, B), 0.1, hot=hot)
    for got in _state(hc, rec):
        assert sc.same_bits(got, np.full(shape, sc.SENTINEL))
    assert _guards_intact(rec) and rec.slot == 1
    assert np.array_equal(_log(rec)[1], np.tile(sc.EMPTY_ROW, (3, 1)))
    if hot:
        assert np.array_equal(rec.d_hot.cpu().numpy(), hc.CylSolidificationRecord.hot_reference(B, None, sc.T_F, shape))
    else:
        assert (rec.d_hot.cpu().numpy() == 1).all()


@pytest.mark.parametrize('shape', sc.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_hot_words_give_the_bits_of_the_null_path_on_the_device(hc, loops, shape):
    Rec = hc.CylSolidificationRecord
    (ref, ref_log), _ = loops[(shape, 'all')]
    g = _grid(hc, shape, sc.case_ids()[sc.SHAPES.index(shape) * 3][2])
    rec = Rec(g, sc.T_F, capacity=sc.NSTEPS, t=sc.T0_CLOCK)
    rec.seed_hot(_dev(g, ref[0]['A']))
    assert np.array_equal(rec.d_hot.cpu().numpy(), Rec.hot_reference(ref[0]['A'], None, sc.T_F, shape))
    for n, r in enumerate(ref):
        rec.record(_dev(g, r['A']), _dev(g, r['B']), sc.DT, hot=True)
        for a, b in zip(_state(hc, rec), r['state']):
            assert sc.same_values(a, b), n
        assert np.array_equal(rec.d_hot.cpu().numpy(), Rec.hot_reference(r['B'], None, sc.T_F, shape)), n
    assert np.array_equal(_log(rec)[1], ref_log) and _guards_intact(rec)


@pytest.mark.parametrize('shape', [(1, 1, 4000), (1, 1, 3999)], ids=lambda s: '%dx%dx%d' % s)
def test_clear_tiles_do_not_read_the_input_on_the_device(hc, shape):
    """the case of test_cyl_solid_cpu.py: three warm stretches on one long z line, every neighbour of a freezing cell in a tile
    whose word is set; A = 1e300 in the tiles whose word is clear changes no bit"""
    import test_cyl_solid_cpu as cpu
    Rec = hc.CylSolidificationRecord
    g = _grid(hc, shape, 0.03)
    A, B = cpu._mostly_cold(shape)
    hot = Rec.hot_reference(A, None, sc.T_F, shape)
    want, front = Rec.record_reference(sc.nan_state(shape), A, B, None, 1.0, 0.5, sc.Grid(shape, 0.03), sc.T_F)
    A2 = A.copy()
    for q in np.flatnonzero(hot == 0):
        A2.reshape(-1)[q * sc.TILE:(q + 1) * sc.TILE] = 1e300
    assert front['cells'] > 10 and (A2 == 1e300).sum() > 1500
    for src in (A, A2):
        rec = Rec(g, sc.T_F, capacity=1, t=1.0)
        rec.seed_hot(_dev(g, A))
        assert np.array_equal(rec.d_hot.cpu().numpy(), hot)
        rec.record(_dev(g, src), _dev(g, B), 0.5, hot=True)
        for a, b in zip(_state(hc, rec), want):
            assert sc.same_values(a, b)
        assert np.array_equal(_log(rec)[1][0], Rec.front_row(front))
        assert np.array_equal(rec.d_hot.cpu().numpy(), Rec.hot_reference(B, None, sc.T_F, shape))


# ---- the plain steps ---------------------------------------------------------------------------------------------------------
def _setup(hc, shape, r_in, zkinds=('neumann0', 'robin'), dt=0.05):
    g = _grid(hc, shape, r_in)
    mat, prm = hc.Material(*MAT), hc.Params(dt, 1.0, 'be')
    wall = hc.RobinR(25.0, 25.0)
    zbc = hc.ZBC(kind_bot=zkinds[0], kind_top=zkinds[1], h_top=15.0, T_inf_top=25.0, T_bot=1425.0, T_top=1380.0)
    return g, mat, prm, wall, zbc


@pytest.mark.parametrize('shape,r_in,zkinds', [((5, 8, 129), 0.03, ('neumann0', 'robin')), ((3, 5, 7), 0.0, ('dirichlet', 'robin')),
                                               ((2, 3, 1024), 0.0, ('neumann0', 'dirichlet'))])   # (a plan's longest line)
def test_step_keyword_is_the_plain_step_then_the_definition(hc, shape, r_in, zkinds):
    """alone, and next to phase=, history= and monitor=: the field and the other objects' results are those of the call
    without solidification=, and the record is the definition on (input, final field)"""
    Rec = hc.CylSolidificationRecord
    g, mat, prm, wall, zbc = _setup(hc, shape, r_in, zkinds)
    law, levels = cc.objects()
    rng = np.random.default_rng(4)
    T = rng.uniform(1200.0, 1650.0, shape)
    act = rng.random(shape) < 0.7
    act[:, rng.random(shape[1:]) < 0.2] = False
    Tm = np.where(act, T, 25.0)
    sgrid = sc.Grid(shape, r_in)

    def others():
        return dict(phase=hc.CylPhaseField(g, mat, law, active=np.zeros(shape, bool)),
                    history=hc.CylThermalHistory(g, levels, capacity=4, t=2.0),
                    monitor=hc.CylFieldMonitor(g, probes=[(0, 0, 0)], capacity=4, t=2.0))

    for step, Tin, a in ((lambda *p, **k: hc.adi_step(*p, **k), T, None),
                         (lambda *p, **k: hc.adi_step_masked(*p, act, **k), Tm, act)):
        plain = np.asarray(step(hc.to_device(Tin), g, mat, prm, wall, zbc))
        assert sc.same_bits(plain, np.asarray(step(hc.to_device(Tin), g, mat, prm, wall, zbc, solidification=None)))
        rec = Rec(g, sc.T_F, capacity=4, t=2.0)
        got = np.asarray(step(hc.to_device(Tin), g, mat, prm, wall, zbc, solidification=rec))
        want, front = Rec.record_reference(sc.nan_state(shape), Tin, plain, a, 2.0, prm.dt, sgrid, sc.T_F)
        assert sc.same_bits(got, plain) and front['cells'] > 0
        for x, y in zip(_state(hc, rec), want):
            assert sc.same_values(x, y)
        assert np.array_equal(_log(rec)[1][0], Rec.front_row(front)) and rec.slot == 1 and rec.t == 2.0 + prm.dt
        assert (rec.d_hot.cpu().numpy() == 1).all() and _guards_intact(rec)        # (the plain step passes no hot words)
        # next to the other three
        o1, o2 = others(), others()
        base = np.asarray(step(hc.to_device(Tin), g, mat, prm, wall, zbc, **o1))
        rec = Rec(g, sc.T_F, capacity=4, t=2.0)
        got = np.asarray(step(hc.to_device(Tin), g, mat, prm, wall, zbc, solidification=rec, **o2))
        assert sc.same_bits(got, base) and not sc.same_bits(base, plain)
        assert sc.same_values(_host(hc, o1['phase'].f), _host(hc, o2['phase'].f))
        for x, y in zip((o1['history'].d_peak, o1['history'].d_t_hi, o1['history'].d_t_lo),
                        (o2['history'].d_peak, o2['history'].d_t_hi, o2['history'].d_t_lo)):
            assert sc.same_values(_host(hc, x), _host(hc, y))
        assert np.array_equal(o1['history']._log_store.cpu().numpy(), o2['history']._log_store.cpu().numpy())
        assert np.array_equal(o1['monitor']._log_store.cpu().numpy(), o2['monitor']._log_store.cpu().numpy())
        want, front = Rec.record_reference(sc.nan_state(shape), Tin, base, a, 2.0, prm.dt, sgrid, sc.T_F)
        for x, y in zip(_state(hc, rec), want):
            assert sc.same_values(x, y)
        assert np.array_equal(_log(rec)[1][0], Rec.front_row(front)) and front['cells'] > 0
    other = _grid(hc, shape, r_in)
    with pytest.raises(ValueError, match='another grid'):
        hc.adi_step(hc.to_device(T), other, mat, prm, wall, zbc, solidification=rec)
    with pytest.raises(TypeError):
        hc.adi_step(hc.to_device(T), g, mat, prm, wall, zbc, solidification=o1['history'])
    assert rec.slot == 1


# ---- the stepper -----------------------------------------------------------------------------------------------------------------
def _recorder_state(hc, r, fields):
    """a recorder's fields, its log and its clock in the form run() and step() must agree on: a run leaves the block at
    (t0, n), single steps at (t0 + (n - 1) dt, 1) -- the time t0 + n dt, the slot and the capacity are what both share"""
    blk = r.d_block.cpu().numpy()
    t0, dt = blk.view(np.float64)[:2]
    return [_host(hc, s) for s in fields] + [r._log_store.cpu().numpy().astype(np.float64),
                                             np.array([t0 + blk[2] * dt, dt, blk[3], blk[4]]),
                                             np.array([r.slot, r.t] + list(r._times))]


def _stepper_state(hc, ph, hist, rec):
    out = _recorder_state(hc, rec, (rec.d_t_solid, rec.d_rate, rec.d_g2))
    if ph is not None:
        out.append(_host(hc, ph.f))
    if hist is not None:
        out += _recorder_state(hc, hist, (hist.d_peak, hist.d_t_hi, hist.d_t_lo))
    return out


@pytest.mark.parametrize('combo', ['alone', 'history', 'phase', 'phase+history'])
@pytest.mark.parametrize('shape,zkinds', [((5, 8, 129), ('neumann0', 'robin')), ((2, 1, 36), ('dirichlet', 'robin'))])
def test_stepper_run_is_step_called_n_times(hc, shape, zkinds, combo):
    Rec = hc.CylSolidificationRecord
    g, mat, prm, wall, zbc = _setup(hc, shape, 0.03, zkinds, dt=0.0625)      # (a dt whose multiples from t = 1 are exact: the
    law, levels = cc.objects()                                               # clocks of run and of step() then agree to the bit)
    rng = np.random.default_rng(6)
    T = rng.uniform(1200.0, 1650.0, shape)

    def fresh():
        ph = hc.CylPhaseField(g, mat, law, T=T) if 'phase' in combo else None
        hist = hc.CylThermalHistory(g, levels, capacity=8, t=1.0) if 'history' in combo else None
        rec = Rec(g, sc.T_F, capacity=8, t=1.0)
        return ph, hist, rec, hc.StagedCylStepper(g, mat, prm, wall, zbc, phase=ph, history=hist, solidification=rec)

    def by_steps(st, ph, hist, rec, T, n):
        cur = hc.to_device(T)
        for _ in range(n):
            cur = st.step(cur)
        return [np.asarray(cur)] + _stepper_state(hc, ph, hist, rec)

    for graph in (True, False):
        for n in ((1, 5) if graph else (5,)):
            ph_r, hist_r, rec_r, st_r = fresh()
            ph_s, hist_s, rec_s, st_s = fresh()
            want = by_steps(st_s, ph_s, hist_s, rec_s, T, n)
            got = [np.asarray(st_r.run(hc.to_device(T), n, graph=graph))] + _stepper_state(hc, ph_r, hist_r, rec_r)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert sc.same_values(a, b), (graph, n)
            assert sc.same_bits(got[0], want[0])
            assert st_r.captures == (1 if graph and n >= 2 else 0) and st_r._graph['Y'] is not None
            assert np.array_equal(rec_r.d_hot.cpu().numpy(), Rec.hot_reference(got[0], None, sc.T_F, shape))
            assert (rec_s.d_hot.cpu().numpy() == 1).all() and _guards_intact(rec_r)
        assert np.isfinite(want[1]).any() and rec_r.front()['cells'].sum() > 0       # (cells froze in these 5 steps)
        # a second run of the objects that did 5 steps, on the same graph, from another field: the words are seeded again (the
        # new field would otherwise meet the words of the old one) and the clocks continue
        T2 = np.random.default_rng(16).uniform(1200.0, 1650.0, shape)
        want = by_steps(st_s, ph_s, hist_s, rec_s, T2, 3)
        got = [np.asarray(st_r.run(hc.to_device(T2), 3, graph=graph, t0=7.5))] + _stepper_state(hc, ph_r, hist_r, rec_r)
        for a, b in zip(got, want):
            assert sc.same_values(a, b), graph
        assert sc.same_bits(got[0], want[0])
        assert st_r.captures == (1 if graph else 0) and rec_r.slot == 8 and rec_r.t == 1.0 + 8 * 0.0625
        assert rec_r.front()['cells'][5:].sum() > 0
    with pytest.raises(TypeError):
        hc.StagedCylStepper(g, mat, prm, wall, zbc, solidification=levels)
    with pytest.raises(ValueError, match='another grid'):
        hc.StagedCylStepper(_grid(hc, shape, 0.03), mat, prm, wall, zbc, solidification=Rec(g, sc.T_F, capacity=1))


def test_stepper_without_the_keyword_is_unchanged(hc):
    shape = (5, 8, 129)
    g, mat, prm, wall, zbc = _setup(hc, shape, 0.03)
    T = np.random.default_rng(8).uniform(300.0, 1650.0, shape)
    st = hc.StagedCylStepper(g, mat, prm, wall, zbc, solidification=None)
    cur = hc.to_device(T)
    for _ in range(3):
        cur = hc.adi_step(cur, g, mat, prm, wall, zbc)
    assert sc.same_bits(np.asarray(st.run(hc.to_device(T), 3)), np.asarray(cur))
    assert sc.same_bits(np.asarray(st.run(hc.to_device(T), 3, graph=False)), np.asarray(cur))
    assert st.captures == 1 and st._graph['Y'] is None and st._graph['key'] == (None, None, None)
    law, levels = cc.objects()
    hist = hc.CylThermalHistory(g, levels, capacity=4)
    st = hc.StagedCylStepper(g, mat, prm, wall, zbc, history=hist)
    st.run(hc.to_device(T), 2)
    assert st._graph['key'] == (None, None, hist.graph_key()) and st.captures == 1
    rec = hc.CylSolidificationRecord(g, sc.T_F, capacity=4)
    key = rec.graph_key()
    assert key[:5] == (sc.T_F, g.R_in, g.dr, g.dphi, g.dz) and rec.d_hot.data_ptr() in key and rec.d_block.data_ptr() in key


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_spiral_deposition_with_the_solidification_record(hc):
    from adi_thermal_fields_amd import waam
    from adi_thermal_fields_amd.phase import PhaseChange
    law = PhaseChange(*cc.SPIRAL_LAW)
    T_f = sc.SPIRAL_T_FREEZE
    ref = sc.spiral_solid_reference()
    assert ref['margin'] > 1e-6                                   # first: no comparison of the reference sits on the level
    grid, fields, masks, f, sol = waam.run_spiral_deposition(hc, *cc.spiral_args(), phase_change=law, solidification=T_f)
    Tmax = max(float(np.max(np.abs(a))) for a in ref['fields'])
    for a, b, ma, mb in zip(fields, ref['fields'], masks, ref['masks']):
        assert np.array_equal(ma, mb)
        assert float(np.max(np.abs(a - b))) / float(np.max(np.abs(b))) <= 1e-10
    # the margin (9e-4 of 1400 K against fields good to 1e-10) guarantees the same cells freeze in the same steps
    want_t, want_rate, want_g2 = ref['state']
    on = np.isfinite(want_t)
    assert on.sum() == 96 and np.array_equal(np.isfinite(sol['t_solid']), on)
    front, rows = sol['front'], np.array(ref['rows'])
    assert front['dropped'] == 0 and len(front['cells']) == len(rows) == 40
    assert np.array_equal(front['cells'], rows[:, 0]) and np.array_equal(front['lo'], rows[:, 1:4])
    assert np.array_equal(front['hi'], rows[:, 4:7])
    assert np.array_equal(front['sum_i'], np.ascontiguousarray(rows[:, 8:10]).view(np.int64)[:, 0])
    assert np.allclose(front['t'], ref['t_end'], rtol=0, atol=1e-12)
    # e = 1e-10 max|T| in A or B.  t_solid = t_n + dt (A - T_f)/(A - B): d/dA + d/dB of it is dt/(A - B) to first order, so e
    # moves the crossing by e dt/(A - B) of the crossing step; the clocks add rounding
    e = 1e-10 * Tmax
    slope, den = ref['slope'][on], ref['den'][on]
    assert np.isfinite(slope).all() and (den >= 8.0).all()
    tol = e * slope + 8 * EPS * np.abs(want_t[on])
    assert (np.abs(sol['t_solid'][on] - want_t[on]) <= tol).all()
    # the rate (A - B)/dt: 2 e / dt, dt = slope (A - B)
    dts = slope * den
    assert (np.abs(sol['cooling_rate'][on] - want_rate[on]) <= 2 * e / dts + 8 * EPS * np.abs(want_rate[on])).all()
    # G: per axis g = gA + fr (gB - gA); a difference quotient errs by 2 e / h (one-sided; central half of it), fr by e/(A - B),
    # and |gB - gA| is at most 2 span / h with span the range of the active field; the norm of the three errors bounds G's
    g = ref['grid']
    hs = np.array([g.dr, g.R_in * g.dphi, g.dz])                    # (R_in dphi: below every r_i dphi)
    span = cc.SPIRAL['Tdep'] - cc.SPIRAL['Tinf']
    per_axis = 2 * e / hs[:, None] + (2 * span / hs[:, None]) * (e / den[None, :])
    tol_G = np.sqrt((per_axis ** 2).sum(axis=0)) + 8 * EPS * np.sqrt(want_g2[on])
    err_G = np.abs(sol['G'][on] - np.sqrt(want_g2[on]))
    print('largest errors: t_solid %.3g s, G %.3g K/m (bar at that cell %.3g)' % (
        float(np.max(np.abs(sol['t_solid'][on] - want_t[on]))), float(np.max(err_G)), float(tol_G[np.argmax(err_G)])))
    assert (err_G <= tol_G).all() and float(np.min(np.sqrt(want_g2[on]))) > 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        assert sc.same_values(sol['R'], sol['cooling_rate'] / sol['G'])
    with pytest.raises(ValueError, match='needs the device loop'):
        waam.run_spiral_deposition(hc, *cc.spiral_args(), solidification=T_f, device_resident=False)
