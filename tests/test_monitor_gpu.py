"""GPU: the FieldMonitor on the device -- adi_monitor_record through FieldMonitor, the `monitor=` argument of
adi_step_numba_coeff / StagedStepper and of the waam loops -- against the definition, FieldMonitor.record_reference, fed with
the fields read back from the same run.

Bars: every word of a row -- probes, counts, extrema, sums -- equal bit for bit (np.array_equal on the int64 patterns, so NaN in
the same places and the sign of a zero included): both sides add in one fixed order that depends on the bricks and the region's
box alone.  The energy test holds the logged heat to (d + 1) eps sum|terms| of math.fsum, d from FieldMonitor.rounding_depth."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import monitor_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


VARIANTS = [(1, None), (1, mc.PADDED[1]), (2, None), (2, mc.PADDED[2]), (3, None), (4, None)]
IDS = ['case1', 'case1_padded', 'case2', 'case2_padded', 'case3', 'case4']


def _pad(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _mark_outside(grid, T):
    """mc.OUTSIDE into every cell of the physical box outside the logical one"""
    L = grid.layout
    full = T.t.as_strided((L.px, L.py, L.pz), (L.sx, L.pz, 1))
    full[L.nx:] = mc.OUTSIDE
    full[:, L.ny:] = mc.OUTSIDE
    full[:, :, L.nz:] = mc.OUTSIDE


def _assert_row(row, want, what):
    assert row.dtype == np.int64 and want.dtype == np.int64 and row.shape == want.shape, what
    bad = np.flatnonzero(row != want)
    assert bad.size == 0, (what, bad.tolist(), row[bad].view(np.float64).tolist(), want[bad].view(np.float64).tolist())


def _monitor(hip, c, grid, mm, capacity=8, **kw):
    extra = hip.to_device(np.array(c['extra'])) if 'extra' in c else None
    return hip.FieldMonitor(grid, probes=c['probes'], regions=c['regions'], capacity=capacity, material_map=mm, extra=extra,
                            **kw)


@pytest.mark.parametrize('n,phys', VARIANTS, ids=IDS)
def test_rows_against_the_definition(mods, monkeypatch, n, phys):
    hip = mods
    _pad(monkeypatch, hip, phys)
    c = mc.case(n)
    grid, mat, packs, mm = mc.setup(hip, c)
    assert grid.layout.pd[:3] == mc.phys_of(c, phys)
    mon = _monitor(hip, c, grid, mm)
    FM = hip.FieldMonitor
    T = hip.to_device(np.array(c['T0']))
    if grid.layout.padded:
        _mark_outside(grid, T)
    prm = hip.Params(mc.DT, mc.THETA)
    mon.record(T, 0.0)                                              # the initial state
    want = [FM.row_of(mc.reference(FM, c, c['T0']))]
    kw = dict(material_map=mm) if mm is not None else {}
    plain = T
    for s in range(3):
        T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=mc.TINF, monitor=mon, **kw)
        plain = hip.adi_step_numba_coeff(plain, grid, mat, prm, packs, Tinf=mc.TINF, **kw)
        assert np.array_equal(np.asarray(T), np.asarray(plain)), s  # the monitor never touches T
        want.append(FM.row_of(mc.reference(FM, c, np.asarray(T))))
    rows, dropped = mon.rows()
    assert dropped == 0 and len(rows) == 4 and mon.slot == 4
    for s, (r, w) in enumerate(zip(rows, want)):
        _assert_row(r, w, 'row %d' % s)
    assert (rows[1:, len(c['probes'])] == rows[0, len(c['probes'])]).all()      # counts are integers: the same mask, the same count
    lo, hi = mon.guards()
    assert (lo == mon.GUARD_WORD).all() and (hi == mon.GUARD_WORD).all()
    # the accessors
    tr, log = mon.traces(), mon.region_log(mat=mat)
    assert tr['T'].shape == (len(c['probes']), 4) and np.allclose(tr['t'], [0.0, mc.DT, 2 * mc.DT, 3 * mc.DT])
    ref = mc.reference(FM, c, np.asarray(T))
    assert np.array_equal(mc.bits(tr['T'][:, -1]), mc.bits(ref['probes']))
    assert np.array_equal(log['cells'][:, -1], ref['cells']) and np.array_equal(mc.bits(log['sum_T'][:, -1]), mc.bits(ref['sum_T']))
    with np.errstate(invalid='ignore', divide='ignore'):
        assert np.array_equal(mc.bits(log['T_mean'][:, -1]), mc.bits(ref['sum_T'] / ref['cells']))
    if mm is not None:
        assert np.array_equal(mc.bits(log['heat'][:, -1]), mc.bits(ref['sum_wT']))
        assert np.array_equal(mc.bits(log['sum_extra'][:, -1]), mc.bits(ref['sum_extra']))
    else:
        assert np.array_equal(mc.bits(log['heat'][:, -1]), mc.bits((mat.rho * mat.cp * grid.dx ** 3) * ref['sum_T']))
        assert 'sum_extra' not in log and 'heat' not in mon.region_log()


def test_directed_values(mods):
    hip = mods
    d = mc.directed()
    grid = hip.Grid3D(*d['shape'], mc.DX, np.array(d['mask']))
    mon = hip.FieldMonitor(grid, probes=d['probes'], regions=d['regions'], capacity=2)
    mon.record(hip.to_device(np.array(d['T'])), 0.0)
    rows, _ = mon.rows()
    FM = hip.FieldMonitor
    _assert_row(rows[0], FM.row_of(FM.record_reference(d['T'], d['mask'], d['probes'], d['regions'])), 'directed')
    log = mon.region_log()
    for r, (lo, hi) in enumerate(d['want']):
        assert mc.bits(log['T_min'][r, 0]) == mc.bits(lo) and mc.bits(log['T_max'][r, 0]) == mc.bits(hi), r
    assert log['cells'][-1, 0] == 1


@pytest.mark.parametrize('n', [2, 4])
def test_c_abi_with_arrays_that_are_only_8_byte_aligned(mods, n):
    """the layout allows 16-byte loads, the field's address does not: the cell-by-cell form, the same bits"""
    import torch
    hip = mods
    from adi_thermal_fields_amd import _lib
    c = mc.case(n)
    assert mc.vec_form(c)
    grid, mat, packs, mm = mc.setup(hip, c)
    mon = _monitor(hip, c, grid, mm)
    L = grid.layout
    raw = torch.zeros(L.numel_padded + 1, dtype=torch.float64, device='cuda')
    t = raw[1:].as_strided(L.shape, L.strides)
    assert t.data_ptr() % 16 == 8
    t.copy_(torch.from_numpy(c['T0']))
    P = lambda x: ctypes.c_void_p(0 if x is None else x.data_ptr())    # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.adi_monitor_record(P(mon.d_block), P(t), P(mon._d_extra), P(None if mm is None else mm._d_ids),
                                           P(grid.d_flags), P(grid.d_bricks), *L.pd, len(mon.regions), mon._h_regions,
                                           len(mon.probes), mon._h_probes, P(mon._d_probes),
                                           0 if mm is None else len(mm.materials), mon._h_weights, P(mon.d_partial),
                                           mon.d_partial.numel(), P(mon.d_log), mon.capacity, stream))
    _lib.check(_lib.lib.adi_history_tick(P(mon.d_block), stream))
    rows, _ = mon.rows()
    FM = hip.FieldMonitor
    assert len(rows) == 1
    _assert_row(rows[0], FM.row_of(mc.reference(FM, c, c['T0'])), 'unaligned')


def test_launch_box_independence(mods):
    """a small region alone (a launch of one brick) and next to the whole grid (a launch of every brick): the same words"""
    hip = mods
    c = mc.case(1)
    grid, mat, packs, _ = mc.setup(hip, c)
    small = c['regions'][2]
    cut = c['regions'][1]
    T = hip.to_device(np.array(c['T0']))
    words = {}
    for name, regions in (('alone', (small,)), ('with_whole', (None, small)), ('cut_alone', (cut,)), ('cut_last', (None, small, cut))):
        mon = hip.FieldMonitor(grid, regions=regions, capacity=1)
        mon.record(T, 0.0)
        rows, _ = mon.rows()
        words[name] = rows[0].reshape(len(regions), 6)
    assert np.array_equal(words['alone'][0], words['with_whole'][1]) and words['alone'][0, 0] > 0
    assert np.array_equal(words['cut_alone'][0], words['cut_last'][2])
    assert np.array_equal(words['alone'][0], words['cut_last'][1])


def test_births_need_no_call(mods):
    """layers born across planes 15 | 16 between steps: probes go from NaN to values, counts grow, every row is the definition's
    on the mask of its step -- and the monitor is never told"""
    import torch
    hip = mods
    FM = hip.FieldMonitor
    shape = (20, 20, 40)
    rng = np.random.default_rng(77)
    full = rng.random(shape) < 0.9
    full[5, 5, :] = True
    grid = hip.Grid3D(*shape, mc.DX, np.zeros(shape, dtype=bool))
    mat = hip.Material(mc.RHO, mc.CP, mc.K)
    L = grid.layout
    d_full = L.to_layout(full, torch.uint8)
    d_act = L.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    bpacks = hip.BirthPacks(grid, mat, robin_h={f: mc.H for f in mc.FACES})
    probes = ((5, 5, 10), (5, 5, 15), (5, 5, 16), (5, 5, 35))
    regions = (None, ((0, 20), (0, 20), (10, 22)))
    mon = FM(grid, probes=probes, regions=regions, capacity=8)
    T = hip.to_device(np.full(shape, mc.TINF))
    prm = hip.Params(mc.DT, mc.THETA)
    mon.record(T, 0.0)                                              # nothing is active: NaN and zero counts
    want_masks = [np.zeros(shape, dtype=bool)]
    fields = [np.asarray(T)]
    for k0, k1, Ts in ((0, 16, 1500.0), (16, 32, 1400.0)):
        hip.birth_planes(T, d_act, d_full, grid, k0, k1, Ts)
        grid.set_mask_device(d_act, max(k0 - 1, 0), min(shape[2], k1 + 1), all_solid=False)
        packs = bpacks.update(k0 - 1, k1 + 1)
        for _ in range(2):
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=mc.TINF, monitor=mon)
            want_masks.append(np.array(grid.mask))
            fields.append(np.asarray(T))
    rows, dropped = mon.rows()
    assert len(rows) == 5 and dropped == 0
    for s, (r, m, F) in enumerate(zip(rows, want_masks, fields)):
        _assert_row(r, FM.row_of(FM.record_reference(F, m, probes, regions)), 'row %d' % s)
    tr, log = mon.traces(), mon.region_log()
    assert np.isnan(tr['T'][:, 0]).all()
    assert np.isfinite(tr['T'][:2, 1:]).all() and np.isnan(tr['T'][2, 1:3]).all() and np.isfinite(tr['T'][2, 3:]).all()
    assert np.isnan(tr['T'][3]).all()
    assert log['cells'][0, 0] == 0 and 0 < log['cells'][0, 1] == log['cells'][0, 2] < log['cells'][0, 3] == log['cells'][0, 4]
    assert log['cells'][0, 4] == int(full[:, :, :32].sum())
    assert np.isnan(log['T_min'][:, 0]).all() and np.isnan(log['T_max'][:, 0]).all()


def _small(hip):
    shape = (20, 20, 40)
    rng = np.random.default_rng(5)
    mask = rng.random(shape) < 0.9
    T0 = np.where(mask, 300.0 + 700.0 * rng.random(shape), mc.OFF)
    grid = hip.Grid3D(*shape, mc.DX, mask)
    mat = hip.Material(mc.RHO, mc.CP, mc.K)
    packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h={f: mc.H for f in mc.FACES})
    return grid, mat, packs, mask, T0


def test_graph_replay_401_steps(mods):
    hip = mods
    grid, mat, packs, mask, T0 = _small(hip)
    prm = hip.Params(mc.DT, mc.THETA)
    spec = dict(probes=((3, 4, 5), (19, 19, 39)), regions=(None, ((2, 18), (1, 19), (3, 35))), capacity=400)
    a, b = hip.FieldMonitor(grid, **spec), hip.FieldMonitor(grid, **spec)
    stepper = hip.StagedStepper(grid, mat, prm, packs, mc.TINF, monitor=a)
    out = stepper.run(hip.to_device(np.array(T0)), 401)
    assert stepper.captures == 1 and len(stepper._graph['key']) == 16
    T = hip.to_device(np.array(T0))
    for _ in range(401):
        T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=mc.TINF, monitor=b)
    assert np.array_equal(np.asarray(out), np.asarray(T))
    (ra, da), (rb, db) = a.rows(), b.rows()
    assert da == db == 1 and ra.shape == rb.shape == (400, a.row_words) and a.slot == 401
    assert np.array_equal(ra, rb)
    spill = lambda m: m.d_log.cpu().numpy().reshape(401, m.row_words)[400]     # noqa: E731
    FM = hip.FieldMonitor
    want = FM.row_of(FM.record_reference(np.asarray(T), mask, spec['probes'], spec['regions']))
    _assert_row(spill(a), want, 'spill row, replayed')              # the step past the capacity went to the spill row
    _assert_row(spill(b), want, 'spill row, single')
    _assert_row(ra[0], FM.row_of(FM.record_reference(np.asarray(hip.adi_step_numba_coeff(
        hip.to_device(np.array(T0)), grid, mat, prm, packs, Tinf=mc.TINF)), mask, spec['probes'], spec['regions'])), 'row 0')
    for m in (a, b):
        lo, hi = m.guards()
        assert (lo == m.GUARD_WORD).all() and (hi == m.GUARD_WORD).all()
    assert a.t == pytest.approx(401 * mc.DT) and len(a.traces()['t']) == 400
    # a second run continues the clock and the slot
    stepper.run(out, 4)
    assert stepper.captures == 1 and a.slot == 405 and a.rows()[1] == 5 and a.t == pytest.approx(405 * mc.DT)
    assert np.array_equal(a.rows()[0], ra)
    a.reset(t=1.0)
    assert a.slot == 0 and a.t == 1.0 and len(a.rows()[0]) == 0


def test_bystanders_are_untouched(mods):
    hip = mods
    grid, mat, packs, mask, T0 = _small(hip)
    prm = hip.Params(mc.DT, mc.THETA)
    lv = hip.HistoryLevels(800.0, 500.0, 900.0)
    res = {}
    for with_mon in (False, True):
        T = hip.to_device(np.array(T0))
        h = hip.ThermalHistory(grid, lv, capacity=16, T=T)
        s = hip.SolidificationRecord(grid, 700.0, T=T)
        kw = dict(monitor=hip.FieldMonitor(grid, probes=((3, 4, 5),), capacity=16)) if with_mon else {}
        stepper = hip.StagedStepper(grid, mat, prm, packs, mc.TINF, history=h, solidification=s, **kw)
        out = stepper.run(T, 7)
        one = hip.adi_step_numba_coeff(out, grid, mat, prm, packs, Tinf=mc.TINF, history=h, solidification=s, **kw)
        pool = h.melt_pool()
        res[with_mon] = [np.asarray(out), np.asarray(one), np.asarray(h.T_peak), np.asarray(h.t_hi), np.asarray(h.t_lo),
                         pool['cells'], pool['lo'], pool['hi'], pool['t'], np.asarray(s.t_solid), np.asarray(s.cooling_rate),
                         np.asarray(s.g2)]
        assert len(stepper._graph['key']) == (16 if with_mon else 15)     # without a monitor the key is what it was
        if with_mon:
            assert kw['monitor'].slot == 8
    for i, (x, y) in enumerate(zip(res[False], res[True])):
        assert np.array_equal(x, y, equal_nan=True), i
    assert np.isfinite(res[True][9]).sum() > 0                      # (cells did freeze: the comparison is not of NaN alone)


def test_energy_audit(mods):
    """an adiabatic body of two materials under a source field that is constant on a sub-box: the logged heat of every step
    within (d + 1) eps sum|w T| of math.fsum over the field read back"""
    hip = mods
    FM = hip.FieldMonitor
    shape = (32, 32, 48)
    rng = np.random.default_rng(31)
    mask = np.ones(shape, dtype=bool)
    mask[20:, 20:, 30:] = False
    ids = np.zeros(shape, dtype=np.uint8)
    ids[:, :, 24:] = 1
    grid = hip.Grid3D(*shape, mc.DX, mask)
    mm = hip.MaterialMap(grid, mc.MATERIALS, ids)                   # no surface loss: adiabatic
    box = ((0, 32), (0, 32), (0, 48))
    mon = FM(grid, regions=(None,), capacity=8, material_map=mm)
    S = np.zeros(shape)
    S[8:16, 8:16, 20:28] = 5.0e9
    T = hip.to_device(np.where(mask, 300.0 + rng.random(shape), mc.OFF))
    prm = hip.Params(mc.DT, mc.THETA)
    w = np.array(FM.weights_of(mm.materials, grid.dx))
    d = FM.rounding_depth(box)
    heats = []
    for s in range(4):
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, Tinf=mc.TINF, S=S, material_map=mm, monitor=mon)
        terms = (w[ids[mask]] * np.asarray(T)[mask]).tolist()
        exact, bound = math.fsum(terms), (d + 1) * mc.EPS * math.fsum(abs(x) for x in terms)
        got = float(mon.region_log()['heat'][0, s])
        print('step %d heat %r fsum %r |diff| %.3e bound %.3e' % (s, got, exact, abs(got - exact), bound))
        assert abs(got - exact) <= bound, (s, got, exact, bound)
        heats.append(got)
    assert all(b > a for a, b in zip(heats, heats[1:]))             # the source heats the body


def test_run_single_track_with_a_monitor(mods):
    """the probe trace of the loop is the field's value at the cell after every step of a twin run stepped by hand"""
    import torch
    hip = mods
    from adi_thermal_fields_amd import waam
    nx, ny, nz = 16, 12, 16
    plate = np.zeros((nx, ny, nz), dtype=bool)
    plate[:, :, :6] = True
    box = (5, 11, 6, 9, 3)
    x0, x1, z0, z1, ncol = box
    mat_args, dt, t_step, T_track = (mc.RHO, mc.CP, mc.K), 0.004, 0.01, 1600.0
    probes = ((8, 0, 7), (8, 2, 7), (8, 1, 3), (8, 8, 7))
    spec = dict(probes=probes, regions=(None, ((x0, x1), (0, ncol), (z0, z1))))
    Tf, traces, log = waam.run_single_track(hip, plate, box, mc.DX, mat_args, mc.H, mc.TINF, T_track, mc.THETA, dt, t_step,
                                            monitor=spec)
    # the twin, by hand
    grid = hip.Grid3D(nx, ny, nz, mc.DX, plate.copy())
    mat = hip.Material(*mat_args)
    T = hip.to_device(np.full((nx, ny, nz), float(mc.TINF)))
    d_mask = grid.layout.to_layout(plate, torch.uint8)
    robin = {f: mc.H for f in mc.FACES}
    n_sub = int(math.ceil(t_step / dt))
    prm = hip.Params(t_step / n_sub, mc.THETA)
    want, cells = [], []
    for yi in range(ncol):
        d_mask[x0:x1, yi:yi + 1, z0:z1] = 1
        grid.set_mask_device(d_mask)
        packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=robin, robin_Tinf=mc.TINF)
        T[x0:x1, yi:yi + 1, z0:z1] = T_track
        for _ in range(n_sub):
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=mc.TINF)
            Th, m = np.asarray(T), np.array(grid.mask)
            want.append([Th[p] if m[p] else np.nan for p in probes])
            cells.append(int(m[x0:x1, 0:ncol, z0:z1].sum()))
    assert np.array_equal(Tf, np.asarray(T))
    want = np.array(want).T
    assert traces['T'].shape == want.shape == (4, ncol * n_sub)
    assert np.array_equal(mc.bits(traces['T']), mc.bits(want))
    assert np.isnan(want[1, :2 * n_sub]).all() and np.isfinite(want[1, 2 * n_sub:]).all() and np.isnan(want[3]).all()
    assert log['cells'][1].tolist() == cells and log['dropped'] == 0 and 'heat' in log
    assert np.allclose(traces['t'], prm.dt * np.arange(1, ncol * n_sub + 1))
