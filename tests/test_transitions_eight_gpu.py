"""GPU: MaterialTransitions with all eight materials, with the changed cells placed at the brick seams and at the
ends of the box, with the values at the edge of `>=`, after runs that are graph replays alone, through the whole step of eight
materials, and together with deposits and a phase field.  Everything is compared bit for bit: T is not written, ids and words are
integers, f comes from the seed's operations.  Inputs, rules and what every shape was built for: tests/transitions_eight_cases.py
(asserted on the CPU by tests/test_transitions_eight_cpu.py, and here again before a launch)."""
import numpy as np
import pytest
import torch

import matmap_eight_cases as m8
import matmap_extras_cases as xc
import transitions_cases as tc
import transitions_eight_cases as ec
from adi_thermal_fields_amd.matmap_extras import MapLossPacks, MapPhaseField, MaterialTransitions
from adi_thermal_fields_amd.monitor import FieldMonitor
from adi_thermal_fields_amd.packs import MaterialMap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _raw(grid, t):
    """every byte of a device field's buffer: the physical box and the padding of its planes"""
    return t.as_strided((grid.layout.numel_padded,), (1,)).view(torch.int64).clone()


def _rig(hip, monkeypatch, name, rules, phase=True, loss=False, ids=None, f=None):
    """grid, map, phase field (f0 loaded) and transitions of the case `name`, held in the box the case names"""
    dims = ec.dims_of(name)
    monkeypatch.setattr(hip, 'recommended_dims', dims)
    c = ec.case(name)
    grid = hip.Grid3D(*c['shape'], ec.DX, c['mask'])
    assert tuple(grid.layout.pd[:3]) == dims(*c['shape'])
    mm = hip.MaterialMap(grid, ec.MATERIALS, np.array(c['ids']) if ids is None else ids, **ec.bc_of(c, loss))
    mph = None
    if phase:
        mph = hip.MapPhaseField(mm, ec.LAWS)
        mph.set_liquid_fraction(c['f0'] if f is None else f)
    tr = hip.MaterialTransitions(mm, rules, phase=mph)
    return c, grid, mm, mph, tr


def _packs_equal(grid, mm, c, ids, what):
    want = MaterialMap.packs_reference(c['mask'], ids, ec.MATERIALS, ec.DX, **ec.bc_of(c))
    for a in range(3):
        assert _bits(grid.layout.to_host(mm.packs[a].d_coeff), want[a].coeff), (what, 'coeff', a)
        assert _bits(grid.layout.to_host(mm.packs[a].d_qflux), want[a].qflux), (what, 'qflux', a)


def _state_equal(grid, mm, mph, tr, c, ids, f, what):
    pd = grid.layout.pd[:3]
    assert np.array_equal(mm.ids, ids), what
    assert np.array_equal(tr.brick_ids.cpu().numpy(), xc.brick_words(c['mask'], ids, pd)), what
    if mph is not None:
        assert tr.brick_ids.data_ptr() == mph.brick_ids.data_ptr()
        assert _bits(np.asarray(mph.liquid_fraction), f), what
        assert np.array_equal(mph.summary.cpu().numpy(), xc.brick_any(f, pd)), what


# ---- 1. the pass against its definition, on every shape ------------------------------------------------------------------------
@pytest.mark.parametrize('phase', [True, False], ids=['phase', 'no_phase'])
@pytest.mark.parametrize('name', list(ec.SHAPES))
def test_apply_is_the_definition_with_eight_materials(hip, monkeypatch, name, phase):
    ec.assert_covered(name)                                 # (on the CPU, before any launch)
    ec.assert_conditions(name)
    c, grid, mm, mph, tr = _rig(hip, monkeypatch, name, ec.RULES8, phase)
    _state_equal(grid, mm, mph, tr, c, c['ids'], c['f0'], 'before')
    _packs_equal(grid, mm, c, c['ids'], 'before')
    T = hip.to_device(c['T'])
    raw = _raw(grid, T.t)
    ids, f, total = c['ids'], (c['f0'] if phase else None), 0
    counts = []
    for n in range(3):                                      # the second hop of the chain, the way back of the cycle
        ids, f, k = ec.reference(ec.RULES8, c['T'], f, c['mask'], ids, c['dir_mask'])
        total += k
        counts.append(k)
        tr.apply(T)
        assert tr.changed == total, (n, tr.changed, total)
        _state_equal(grid, mm, mph, tr, c, ids, f, 'pass %d' % n)
        _packs_equal(grid, mm, c, ids, 'pass %d' % n)
    print('%s: cells changed in three passes: %s' % (name, counts))
    assert all(k > 0 for k in counts)
    assert torch.equal(_raw(grid, T.t), raw)                # no byte of T changed, padding included


# ---- 2. values at the edge of the comparison --------------------------------------------------------------------------------------
@pytest.mark.parametrize('phase', [True, False], ids=['phase', 'no_phase'])
def test_infinities_nan_signed_zeros_and_a_negative_threshold(hip, monkeypatch, phase):
    c, grid, mm, mph, tr = _rig(hip, monkeypatch, 'odd_row', ec.RULES8_EDGE, phase)
    T_host, cells = ec.edge_field(c)
    ids1, f1, n1 = ec.reference(ec.RULES8_EDGE, T_host, c['f0'] if phase else None, c['mask'], c['ids'], c['dir_mask'])
    T = hip.to_device(T_host)
    raw = _raw(grid, T.t)
    tr.apply(T)
    got_ids = mm.ids
    got_f = np.asarray(mph.liquid_fraction) if phase else np.zeros(c['shape'])
    print({what: (int(got_ids[p]), float(got_f[p])) for what, p in cells.items()})
    assert tr.changed == n1 > 100
    _state_equal(grid, mm, mph, tr, c, ids1, f1, 'edge values')
    _packs_equal(grid, mm, c, ids1, 'edge values')
    assert torch.equal(_raw(grid, T.t), raw)
    # the planted cells, by name: +inf changes (f = 1 under a law, 0 without), -inf and NaN do not, both zeros are at -0.0
    for what in ('zero_plus', 'zero_minus', 'inf_no_law'):
        assert got_ids[cells[what]] == 4 and got_f[cells[what]] == 0.0, what
    for what in ('tiny_minus', 'minus_inf_0', 'nan_0'):
        assert got_ids[cells[what]] == 0, what
    assert got_ids[cells['at_negative']] == 6 and got_ids[cells['inf_5']] == 6 and got_ids[cells['inf_law']] == 7
    if phase:
        assert got_f[cells['inf_5']] == 1.0 and got_f[cells['inf_law']] == 1.0
    for what in ('below_negative', 'minus_inf_5', 'nan_5'):
        assert got_ids[cells[what]] == 5, what
    for what in ('minus_inf_3', 'nan_3'):
        assert got_ids[cells[what]] == 3, what
    assert got_ids[cells['inf_off_mask']] == c['ids'][cells['inf_off_mask']]


# ---- 3. a run that is graph replays alone ---------------------------------------------------------------------------------------
RUN_SHAPE = (24, 20, 16)


def _run_rig(hip):
    """the rig of tests/test_transitions_gpu.py: a dense plate (planes 0 - 7) under a powder layer (planes 8 - 11) with a copper
    bar through both and a source on the powder; the definitions give 10, 42, 68, 88, 104, 106, 118, 142, 148 changed cells
    after its first nine steps"""
    mask = np.zeros(RUN_SHAPE, bool)
    mask[:, :, :12] = True
    ids = np.full(RUN_SHAPE, 1, np.uint8)
    ids[:, :, 8:] = 0
    ids[:3, :, :] = 2
    grid = hip.Grid3D(*RUN_SHAPE, tc.DX, mask)
    mm = hip.MaterialMap(grid, tc.MATERIALS, ids, robin_h=40.0)
    T0 = np.where(mask, 1300.0, tc.TINF)
    mph = hip.MapPhaseField(mm, tc.LAWS, T=hip.to_device(T0))
    tr = hip.MaterialTransitions(mm, tc.RULES['powder'], phase=mph)
    src = hip.GoldakSource(power=30000.0, eta=0.8, a=4e-3, b=4e-3, c_f=4e-3, c_r=6.4e-3, f_f=0.6, origin=(9e-3, 10e-3, 12e-3),
                           velocity=0.08, travel_axis=0, travel_sign=1, depth_axis=2)
    prm = hip.Params(4e-3, 0.5)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, tc.TINF, material_map=mm, source=hip.MapSource(mm, src), phase=mph,
                           transitions=tr)
    return dict(grid=grid, mm=mm, mph=mph, tr=tr, st=st, prm=prm, T0=T0, ids=ids, mask=mask)


@pytest.mark.parametrize('graph,nsteps', [(True, 4), (False, 4), (True, 5)], ids=['replays_alone', 'plain', 'replays_and_a_step'])
def test_ids_on_the_host_after_every_run(hip, graph, nsteps):
    """run(T, 4) on a captured graph calls no Python between its steps, so nothing but run() itself can tell the map that the
    device id field moved on.  Before StagedStepper.run called MaterialTransitions.after_replay the second `mm.ids` of the first
    form returned the copy made after the first run (88 changed cells where the device held 142)."""
    a, b = _run_rig(hip), _run_rig(hip)
    dt = a['prm'].dt
    Ta, Tb, t0 = hip.to_device(a['T0']), hip.to_device(b['T0']), 0.0
    seen = []
    for run in range(2):
        Ta = a['st'].run(Ta, nsteps, graph=graph, t0=t0)
        for i in range(nsteps):
            Tb = b['st'].step(Tb, t=t0 + i * dt)
        t0 += nsteps * dt
        assert a['st'].captures == (1 if graph else 0)
        ids_a, ids_b = a['mm'].ids, b['mm'].ids             # (reading mm.ids after the first run is part of the sequence)
        changed = int((ids_b != b['ids']).sum())
        seen.append(changed)
        print('run %d (%s, %d steps): host ids differ from the start in %d cells, the twin in %d, tr.changed %d'
              % (run, 'graph' if graph else 'plain', nsteps, int((ids_a != a['ids']).sum()), changed, a['tr'].changed))
        assert changed == b['tr'].changed and (run == 0 or changed > seen[0])      # cells change in the second run too
        assert np.array_equal(ids_a, ids_b), 'run %d' % run
        assert int((ids_a != a['ids']).sum()) == a['tr'].changed == changed
        assert _bits(np.asarray(Ta), np.asarray(Tb))
        assert torch.equal(a['tr'].brick_ids, b['tr'].brick_ids)
        assert _bits(np.asarray(a['mph'].liquid_fraction), np.asarray(b['mph'].liquid_fraction))
    assert seen[0] > 0


# ---- 4. eight materials through the step ------------------------------------------------------------------------------------------
REGIONS = [((0, 33), (0, 33), (0, 34)), ((10, 22), (10, 22), (10, 22)), ((16, 33), (0, 16), (16, 34))]


def _step_rig(hip, monkeypatch, transitions=True, ids=None, f=None, T=None):
    c, grid, mm, mph, tr = _rig(hip, monkeypatch, 'seams', ec.RULES8, True, loss=True, ids=ids, f=f)
    prm = hip.Params(0.3 * ec.DX ** 2 / m8.ALPHA_MAX, 0.5)
    mon = hip.FieldMonitor(grid, regions=REGIONS, capacity=16, material_map=mm)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, ec.TINF, material_map=mm,
                           surface_loss=hip.MapLossPacks(mm, xc.LOSSES8, ec.TINF), phase=mph,
                           transitions=tr if transitions else None, monitor=mon)
    return dict(c=c, grid=grid, mm=mm, mph=mph, tr=tr, st=st, mon=mon, T=hip.to_device(c['T'] if T is None else T))


def _same_rigs(a, b, what):
    assert np.array_equal(a['mm'].ids, b['mm'].ids), what
    assert _bits(np.asarray(a['mph'].liquid_fraction), np.asarray(b['mph'].liquid_fraction)), what
    assert torch.equal(a['tr'].brick_ids, b['tr'].brick_ids) and torch.equal(a['mph'].summary, b['mph'].summary), what
    for p, q in zip(a['mm'].packs, b['mm'].packs):
        assert torch.equal(_raw(a['grid'], p.d_coeff), _raw(b['grid'], q.d_coeff)), what
        assert torch.equal(_raw(a['grid'], p.d_qflux), _raw(b['grid'], q.d_qflux)), what


def test_one_step_of_eight_materials_with_loss_phase_and_a_monitor(hip, monkeypatch):
    ec.assert_conditions('seams')
    a, z = _step_rig(hip, monkeypatch), _step_rig(hip, monkeypatch, transitions=False)
    c, grid, mm, mph, tr = a['c'], a['grid'], a['mm'], a['mph'], a['tr']
    T1, T1z = a['st'].step(a['T']), z['st'].step(z['T'])
    assert _bits(np.asarray(T1), np.asarray(T1z))           # T is not written by the pass
    f_step = np.asarray(z['mph'].liquid_fraction)
    ids1, f1, n1 = ec.reference(ec.RULES8, np.asarray(T1z), f_step, c['mask'], c['ids'], c['dir_mask'])
    print('seams: %d cells change in the step; from %s' % (n1, {m: int(((ids1 != c['ids']) & (c['ids'] == m)).sum())
                                                               for m in ec.RULED}))
    assert tr.changed == n1 > 1000 and z['tr'].changed == 0
    assert all(((ids1 != c['ids']) & (c['ids'] == m)).any() for m in ec.RULED)
    _state_equal(grid, mm, mph, tr, c, ids1, f1, 'with transitions')
    _state_equal(z['grid'], z['mm'], z['mph'], z['tr'], c, c['ids'], f_step, 'without')
    # the monitor weighs the heat content with the ids the step left
    w = FieldMonitor.weights_of(mm.materials, ec.DX)
    want = FieldMonitor.record_reference(np.asarray(T1), c['mask'], [], REGIONS, weights=w, ids=ids1)['sum_wT']
    old = FieldMonitor.record_reference(np.asarray(T1), c['mask'], [], REGIONS, weights=w, ids=c['ids'])['sum_wT']
    assert _bits(a['mon'].region_log()['heat'][:, 0], want) and not _bits(want, old)
    # a changed cell's coefficients are the zeros of the robin_h=None build until the next loss update; its fluxes those of the
    # new id
    changed = ids1 != c['ids']
    co = MapLossPacks.coeff_reference(c['T'], c['mask'], c['ids'], ec.MATERIALS, ec.DX, xc.LOSSES8, ec.TINF)
    ref = MaterialMap.packs_reference(c['mask'], ids1, ec.MATERIALS, ec.DX, **ec.bc_of(c, True))
    for ax in range(3):
        assert _bits(grid.layout.to_host(mm.packs[ax].d_coeff), np.where(changed, 0.0, co[ax])), ax
        assert _bits(grid.layout.to_host(mm.packs[ax].d_qflux), ref[ax].qflux), ax
    # the step after it is the step of a rig built anew around the same (T, f, ids)
    T2 = a['st'].step(T1)
    n = _step_rig(hip, monkeypatch, ids=ids1, f=f1, T=np.asarray(T1))
    T2n = n['st'].step(n['T'])
    assert _bits(np.asarray(T2), np.asarray(T2n)) and not _bits(np.asarray(T2), np.asarray(T1))
    assert tr.changed - n1 == n['tr'].changed > 0
    _same_rigs(a, n, 'the second step')


def test_a_run_of_eight_materials_is_four_steps(hip, monkeypatch):
    a, b = _step_rig(hip, monkeypatch), _step_rig(hip, monkeypatch)
    Tb, counts = b['T'], []
    for _ in range(4):
        Tb = b['st'].step(Tb)
        counts.append(b['tr'].changed)
    print('seams: cells changed after each of four steps:', counts)
    assert len(set(counts)) == 4
    Ta = a['st'].run(a['T'], 4)
    assert a['st'].captures == 1 and _bits(np.asarray(Ta), np.asarray(Tb))
    assert a['tr'].changed == counts[-1]
    _same_rigs(a, b, 'after four steps')
    assert _bits(a['mon'].region_log()['heat'], b['mon'].region_log()['heat'])
    # the host's view after replays alone, and the state against the definitions from the start
    ids_now = a['mm'].ids
    assert int((ids_now != a['c']['ids']).sum()) <= counts[-1] and (ids_now != a['c']['ids']).any()
    assert np.array_equal(a['tr'].brick_ids.cpu().numpy(), xc.brick_words(a['c']['mask'], ids_now, a['grid'].layout.pd[:3]))
    assert (ids_now[~a['c']['mask'] | a['c']['dir_mask']] == a['c']['ids'][~a['c']['mask'] | a['c']['dir_mask']]).all()


# ---- 5. deposits, a phase field and transitions together ----------------------------------------------------------------------------
def test_deposits_a_phase_field_and_transitions_together(hip):
    """plate (0, no law), wire as deposited (1) and wire that was molten once (2); wire -> molten wire at 1280, below the 1800 the
    bead is born with.  Counted from the NumPy definitions, 130 of the 139 newborn cells change, each in the step that follows
    its deposit (the run has no heat input: a cell that did not change then only cools); 36 of them touch the plate.  Every
    brick of the 24 x 20 x 12 box holds plate cells, so no id-set word is ever empty: the word that goes from empty to non-empty
    is the summary's (the plate has no law, f = 0 until the first bead), and the id-set words gain the bits of 1 and 2."""
    import bead_cases as bc
    import matmap_deposit_cases as dc
    from adi_thermal_fields_amd.deposition import PathDeposit
    T_BORN, T_AT = 1800.0, 1280.0
    laws = (None, hip.PhaseChange(2.0e5, 1300.0, 1360.0), hip.PhaseChange(2.1e5, 1500.0, 1560.0))
    rules = (None, (2, T_AT), None)
    robin = {face: dc.H for face in dc.ROBIN}
    path, bead, plate, dt, steps = dc.raster()
    shape, dx = dc.SHAPE, bc.DX
    mask, ids, f = plate.copy(), dc.plate_ids(plate), np.zeros(shape)
    grid = hip.Grid3D(*shape, dx, plate)
    pd = grid.layout.pd[:3]
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=robin)
    T = hip.to_device(np.full(shape, dc.TINF))
    mph = hip.MapPhaseField(mm, laws, T=T)
    tr = hip.MaterialTransitions(mm, rules, phase=mph)
    prm = hip.Params(dt, dc.THETA)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, dc.TINF, material_map=mm, phase=mph, transitions=tr)
    dep = hip.PathDeposit(grid, path.on_device(), bead, T_BORN, material_map=mm, material_id=dc.WIRE)
    near_plate = np.zeros(shape, bool)
    near_plate[:, :, 1:] = plate[:, :, :-1]                 # (the plate is planes 0 - 3: the cells of plane 4 touch it)
    assert not mph.summary.cpu().numpy().any()
    words0 = tr.brick_ids.cpu().numpy().copy()
    stamped, total, steps_with_changes, touching, summary_filled = 0, 0, 0, 0, 0

    def check(what):
        assert np.array_equal(grid.d_mask.cpu().numpy().astype(bool), mask), what
        assert np.array_equal(mm.ids, ids), what
        assert _bits(np.asarray(mph.liquid_fraction), f), what
        assert np.array_equal(tr.brick_ids.cpu().numpy(), xc.brick_words(mask, ids, pd)), what
        assert np.array_equal(mph.summary.cpu().numpy(), xc.brick_any(f, pd)), what
        assert tr.changed == total, what

    for n, (t, d) in enumerate(steps):
        prm.dt = d
        rng = dep.deposit(T, t, d)
        born = PathDeposit.reference(path, bead, shape, dx, t, d, active=mask)
        assert (rng is None) == (not born.any())
        if rng is not None:
            stamped += 1
            mm.update(*rng)
            with pytest.raises(ValueError, match='sync_mask'):
                st.step(T, t=t)                             # before the two syncs
            with pytest.raises(ValueError, match=r'MapPhaseField: .*sync_mask\(T\)'):
                tr.sync_mask()                              # the phase's sync comes first
            mph.sync_mask(T)
            with pytest.raises(ValueError, match=r'MaterialTransitions: .*sync_mask\(\)'):
                st.step(T, t=t)
            tr.sync_mask()
            T_host = np.asarray(T)
            mask = mask | born
            ids = dc.stamp(ids, born, dc.WIRE)
            f = np.where(born, MapPhaseField.f_eq_of(laws, T_host, born, ids), f)
            assert (T_host[born] == T_BORN).all()
            if stamped == 1:                                # (every summary word was 0 before the first bead)
                summary_filled = int((mph.summary.cpu().numpy() != 0).sum())
        check('step %d, after the deposit' % n)
        # the step of a rig built anew around the downloaded state, without transitions
        T_host = np.asarray(T)
        g2 = hip.Grid3D(*shape, dx, mask.copy())
        mm2 = hip.MaterialMap(g2, dc.MATERIALS, ids.copy(), robin_h=robin)
        mph2 = hip.MapPhaseField(mm2, laws)
        mph2.set_liquid_fraction(f)
        T2 = hip.StagedStepper(g2, mm2.mat, hip.Params(d, dc.THETA), mm2.packs, dc.TINF, material_map=mm2,
                               phase=mph2).step(hip.to_device(T_host), t=t)
        T = st.step(T, t=t)
        assert _bits(np.asarray(T), np.asarray(T2)), 'step %d' % n
        ids1, f, k = MaterialTransitions.apply_reference(rules, np.asarray(T2), np.asarray(mph2.liquid_fraction), mask, ids, None,
                                                         laws)
        changed = ids1 != ids
        assert not (changed & plate).any()
        total += k
        steps_with_changes += int(k > 0)
        touching += int((changed & near_plate).sum())
        ids = ids1
        check('step %d, after the step' % n)
        want = MaterialMap.packs_reference(mask, ids, dc.MATERIALS, dx, robin_h=robin)
        for ax in range(3):
            assert _bits(grid.layout.to_host(mm.packs[ax].d_coeff), want[ax].coeff), (n, ax)
    words1 = tr.brick_ids.cpu().numpy()
    print('%d deposits stamped cells; %d newborn cells changed in %d steps, %d of them touch the plate; %d summary words filled; '
          'id-set words %s -> %s' % (stamped, total, steps_with_changes, touching, summary_filled, words0, words1))
    assert stamped >= 2 and total > 0 and steps_with_changes >= 2 and touching >= 1 and summary_filled >= 1
    assert ((words1 & ~words0) & 0b110 == 0b110).any() and (ids[mask & ~plate] != 0).all() and (ids[mask & ~plate] == 1).any()
