"""GPU: cells of a MaterialMap that change their material when they get hot enough (MaterialTransitions).  The pass
against its definition, the step with it against the step without it followed by the definition, StagedStepper's graph against
plain steps, the combination with every other part of the step, and freshness.  Everything is compared bit for bit: T is not
written and f comes from the seed's operations.  Inputs and the coverage condition: tests/transitions_cases.py."""
import numpy as np
import pytest
import torch

import matmap_extras_cases as xc
import transitions_cases as tc
from adi_thermal_fields_amd.matmap_extras import MapLossPacks, MaterialTransitions
from adi_thermal_fields_amd.monitor import FieldMonitor
from adi_thermal_fields_amd.packs import MaterialMap

pytestmark = pytest.mark.gpu

PADDED = lambda nx, ny, nz: (nx + 1, ny + 3, nz + 2)        # noqa: E731  (37 x 21 x 50 in a box of 38 x 24 x 52)
UNPADDED = lambda nx, ny, nz: (nx, ny, nz)                  # noqa: E731  (20 x 18 x 35 as it is: rows of 35 cells)


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _raw(t):
    """the bytes of a device field, padding included"""
    return t.contiguous().view(torch.int64).clone()


def _rig(hip, monkeypatch, name, rules, phase=True, loss=False, ids=None, f=None):
    """grid, map, phase field (f0 loaded) and transitions of the case `name`"""
    if name != 'bricks':
        monkeypatch.setattr(hip, 'recommended_dims', PADDED if name == 'padded' else UNPADDED)
    c = tc.case(name)
    grid = hip.Grid3D(*c['shape'], tc.DX, c['mask'])
    pz = grid.layout.pd[2]
    assert (name == 'padded') == grid.layout.padded and (pz % 2 == 1) == (name == 'odd')
    mm = hip.MaterialMap(grid, tc.MATERIALS, np.array(c['ids']) if ids is None else ids, **tc.bc_of(c, loss))
    mph = None
    if phase:
        mph = hip.MapPhaseField(mm, tc.LAWS)
        mph.set_liquid_fraction(c['f0'] if f is None else f)
    tr = hip.MaterialTransitions(mm, rules, phase=mph)
    return c, grid, mm, mph, tr


def _packs_equal(grid, mm, c, ids, loss=False):
    want = MaterialMap.packs_reference(c['mask'], ids, tc.MATERIALS, tc.DX, **tc.bc_of(c, loss))
    for a in range(3):
        assert _bits(grid.layout.to_host(mm.packs[a].d_coeff), want[a].coeff), ('coeff', a)
        assert _bits(grid.layout.to_host(mm.packs[a].d_qflux), want[a].qflux), ('qflux', a)


def _state_equal(grid, mm, mph, tr, c, ids, f, what):
    pd = grid.layout.pd[:3]
    assert np.array_equal(mm.ids, ids), what
    assert np.array_equal(tr.brick_ids.cpu().numpy(), xc.brick_words(c['mask'], ids, pd)), what
    if mph is not None:
        assert tr.brick_ids.data_ptr() == mph.brick_ids.data_ptr()
        assert _bits(np.asarray(mph.liquid_fraction), f), what
        assert np.array_equal(mph.summary.cpu().numpy(), xc.brick_any(f, pd)), what


# ---- 1. the pass against its definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rules,phase', [('powder', True), ('chain', True), ('powder', False)])
@pytest.mark.parametrize('name', list(tc.SHAPES))
def test_apply_is_the_definition(hip, monkeypatch, name, rules, phase):
    r = tc.RULES[rules]
    tc.assert_covered(tc.case(name), r, '%s/%s' % (name, rules))            # (on the CPU, before any launch)
    c, grid, mm, mph, tr = _rig(hip, monkeypatch, name, r, phase)
    _state_equal(grid, mm, mph, tr, c, c['ids'], c['f0'], 'before')
    _packs_equal(grid, mm, c, c['ids'])
    T_host = np.array(c['T'])
    T_host[6, 6, 6] = np.nan                                # (a powder cell that was hot: a NaN never is)
    T = hip.to_device(T_host)
    raw = _raw(T.t)
    f0 = c['f0'] if phase else None
    ids1, f1, n1 = tc.reference(r, T_host, f0, c['mask'], c['ids'], c['dir_mask'])
    assert n1 > 50 and ids1[6, 6, 6] == 0
    tr.apply(T)
    assert torch.equal(_raw(T.t), raw)                      # no byte of T changed
    assert tr.changed == n1
    _state_equal(grid, mm, mph, tr, c, ids1, f1, 'first pass')
    _packs_equal(grid, mm, c, ids1)
    # a second pass from the state the first left: nothing but the second hop of a chain
    ids2, f2, n2 = tc.reference(r, T_host, f1, c['mask'], ids1, c['dir_mask'])
    assert (n2 > 0) == (rules == 'chain')
    tr.apply(T)
    assert tr.changed == n1 + n2
    _state_equal(grid, mm, mph, tr, c, ids2, f2, 'second pass')
    _packs_equal(grid, mm, c, ids2)
    tr.reset_count()
    assert tr.changed == 0
    # without Dirichlet cells given or built in: the hot ones change too
    if name == 'odd' and not phase:
        mm2 = hip.MaterialMap(grid, tc.MATERIALS, np.array(c['ids']), neumann=c['neumann'], robin_h=c['robin_h'])
        tr2 = hip.MaterialTransitions(mm2, r)
        tr2.apply(T)
        ids3, _, n3 = tc.reference(r, T_host, None, c['mask'], c['ids'], None)
        assert tr2.changed == n3 > n1 and np.array_equal(mm2.ids, ids3)


# ---- 2. the id sets this object owns, without a phase --------------------------------------------------------------------------
def test_own_words_after_construction_a_birth_and_a_deposit(hip):
    import matmap_cases as mc
    import matmap_deposit_cases as dc
    shape = (20, 18, 35)
    full = np.random.default_rng(4).random(shape) > 0.2
    ids = dc.random_ids(shape, 9, 4)
    grid = hip.Grid3D(*shape, tc.DX, np.zeros(shape, bool))
    pd = grid.layout.pd[:3]
    T = hip.to_device(np.full(shape, 300.0))               # (and births at 500: below every threshold)
    d_full = grid.layout.to_layout(full, torch.uint8)
    d_act = grid.layout.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    mm = hip.MaterialMap(grid, tc.MATERIALS, ids, robin_h=50.0)
    tr = hip.MaterialTransitions(mm, tc.RULES['powder'])
    assert not tr.brick_ids.cpu().numpy().any()             # an empty mask: every set is empty
    for ks, ke in ((0, 17), (17, 20)):
        hip.birth_planes(T, d_act, d_full, grid, ks, ke, 500.0)
        grid.set_mask_device(d_act, max(ks - 1, 0), ke + 1, all_solid=False)
        mm.update(ks - 1, ke + 1)
        with pytest.raises(ValueError, match=r'MaterialTransitions: .*sync_mask\(\)'):
            tr.apply(T)
        tr.sync_mask()
        now = np.zeros(shape, bool)
        now[:, :, :ke] = full[:, :, :ke]
        assert np.array_equal(grid.d_mask.cpu().numpy().astype(bool), now)
        assert np.array_equal(tr.brick_ids.cpu().numpy(), xc.brick_words(now, ids, pd)) and tr.brick_ids.cpu().numpy().any()
        tr.apply(T)
        assert tr.changed == 0
    # a PathDeposit's stamp
    path, bead, plate, dt, steps = dc.raster()
    ids = dc.plate_ids(plate)
    grid = hip.Grid3D(*dc.SHAPE, mc.DX, plate)
    pd = grid.layout.pd[:3]
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=50.0)
    tr = hip.MaterialTransitions(mm, ((1, 5000.0), None, None))
    assert np.array_equal(tr.brick_ids.cpu().numpy(), xc.brick_words(plate, ids, pd))
    T = hip.to_device(np.full(dc.SHAPE, 300.0))
    dep = hip.PathDeposit(grid, path.on_device(), bead, 1800.0, material_map=mm, material_id=dc.WIRE)
    stamped = 0
    for t, d in steps[:5]:
        rng = dep.deposit(T, t, d)
        if rng is None:
            continue
        stamped += 1
        mm.update(*rng)
        with pytest.raises(ValueError, match=r'MaterialTransitions: .*sync_mask\(\)'):
            tr.apply(T)
        tr.sync_mask()
        now = grid.d_mask.cpu().numpy().astype(bool)
        assert np.array_equal(tr.brick_ids.cpu().numpy(), xc.brick_words(now, mm.ids, pd))
    assert stamped >= 2 and (now & ~plate).any() and (mm.ids[now & ~plate] == dc.WIRE).all()


# ---- 3. one step ---------------------------------------------------------------------------------------------------------------
def _dt(cfl=0.3):
    return cfl * tc.DX ** 2 / max(k / (rho * cp) for rho, cp, k in tc.MATERIALS)


@pytest.mark.parametrize('form', ['numpy', 'field', 'stepper'])
@pytest.mark.parametrize('name,rules,phase', [('odd', 'chain', True), ('padded', 'powder', True), ('bricks', 'powder', False)])
def test_one_step_is_the_step_without_it_then_the_definition(hip, monkeypatch, name, rules, phase, form):
    r = tc.RULES[rules]
    prm = hip.Params(_dt(), 0.5)

    def one(tr_on):
        c, grid, mm, mph, tr = _rig(hip, monkeypatch, name, r, phase)
        kw = dict(material_map=mm, phase=mph, transitions=tr if tr_on else None)
        if form == 'stepper':
            out = hip.StagedStepper(grid, mm.mat, prm, mm.packs, tc.TINF, **kw).step(hip.to_device(c['T']))
        else:
            T0 = np.array(c['T']) if form == 'numpy' else hip.to_device(c['T'])
            out = hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, tc.TINF, **kw)
            assert isinstance(out, np.ndarray) == (form == 'numpy')
        return c, grid, mm, mph, tr, np.asarray(out)
    c, grid, mm, mph, tr, T1 = one(True)
    _, grid0, mm0, mph0, tr0, T0 = one(False)
    assert _bits(T1, T0)                                    # T is not written by the pass
    f_step = np.asarray(mph0.liquid_fraction) if phase else None
    ids1, f1, n1 = tc.reference(r, T0, f_step, c['mask'], c['ids'], c['dir_mask'])
    print('%s/%s/%s: %d cells change in the step' % (name, rules, form, n1))
    assert n1 > 50 and tr.changed == n1 and tr0.changed == 0
    _state_equal(grid, mm, mph, tr, c, ids1, f1, 'with transitions')
    _packs_equal(grid, mm, c, ids1)
    _state_equal(grid0, mm0, mph0, tr0, c, c['ids'], f_step, 'without')
    _packs_equal(grid0, mm0, c, c['ids'])


# ---- 4. StagedStepper.run: the pass inside the graph --------------------------------------------------------------------------------
RUN_SHAPE = (24, 20, 16)


def _run_rig(hip, power=30000.0):
    """dense plate (planes 0 - 7) under a powder layer (planes 8 - 11) with a copper bar through both; a source on the powder"""
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
    # (the NumPy definitions give 10, 42, 68, 88, 104, 106, 118, 142, 148 changed cells after the nine steps of this rig)
    src = hip.GoldakSource(power=power, eta=0.8, a=4e-3, b=4e-3, c_f=4e-3, c_r=6.4e-3, f_f=0.6, origin=(9e-3, 10e-3, 12e-3),
                           velocity=0.08, travel_axis=0, travel_sign=1, depth_axis=2)
    prm = hip.Params(4e-3, 0.5)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, tc.TINF, material_map=mm, source=hip.MapSource(mm, src), phase=mph,
                           transitions=tr)
    return dict(grid=grid, mm=mm, mph=mph, tr=tr, st=st, prm=prm, T0=T0, ids=ids, mask=mask)


def _steps(hip, rig, T, n, t0=0.0):
    counts = []
    for i in range(n):
        T = rig['st'].step(T, t=t0 + i * rig['prm'].dt)
        counts.append(rig['tr'].changed)
    return T, counts


def _same_state(a, b, what):
    assert np.array_equal(a['mm'].ids, b['mm'].ids), what
    assert _bits(np.asarray(a['mph'].liquid_fraction), np.asarray(b['mph'].liquid_fraction)), what
    assert torch.equal(a['tr'].brick_ids, b['tr'].brick_ids) and torch.equal(a['mph'].summary, b['mph'].summary), what
    assert a['tr'].changed == b['tr'].changed, what
    for p, q in zip(a['mm'].packs, b['mm'].packs):
        assert torch.equal(_raw(p.d_coeff), _raw(q.d_coeff)) and torch.equal(_raw(p.d_qflux), _raw(q.d_qflux)), what


def test_run_with_graph_replay_is_nine_steps(hip):
    a, b = _run_rig(hip), _run_rig(hip)
    Tb, counts = _steps(hip, b, hip.to_device(b['T0']), 9)
    print('cells changed after each of nine steps:', counts)
    assert counts[-1] > 100 and len(set(counts)) >= 4       # cells change during the run, in several of its steps
    Ta = a['st'].run(hip.to_device(a['T0']), 9)
    assert a['st'].captures == 1
    assert _bits(np.asarray(Ta), np.asarray(Tb))
    _same_state(a, b, 'after nine steps')
    ids_now = a['mm'].ids
    assert (ids_now != a['ids']).sum() == counts[-1] and (ids_now[a['ids'] != 0] == a['ids'][a['ids'] != 0]).all()
    _packs = MaterialMap.packs_reference(a['mask'], ids_now, tc.MATERIALS, tc.DX, robin_h=40.0)
    assert _bits(a['grid'].layout.to_host(a['mm'].packs[2].d_coeff), _packs[2].coeff)
    # a second run from where the first ended: nothing is recaptured, and the graph goes on changing the same id field
    Ta2 = a['st'].run(Ta, 9, t0=9 * a['prm'].dt)
    Tb2, counts2 = _steps(hip, b, Tb, 9, t0=9 * b['prm'].dt)
    assert a['st'].captures == 1 and _bits(np.asarray(Ta2), np.asarray(Tb2)) and counts2[-1] > counts[-1]
    _same_state(a, b, 'after eighteen steps')


def test_the_warm_up_of_run_leaves_ids_packs_f_and_words_as_they_were(hip):
    """run(T, 2) takes four warm-up steps before it captures: they change more cells than two steps do, and all of that is put
    back -- the id field, the words, the counter, the packs (MaterialMap.update) and, by the phase's own snapshot, f"""
    a, b, w = _run_rig(hip), _run_rig(hip), _run_rig(hip)
    _, four = _steps(hip, w, hip.to_device(w['T0']), 4)
    Tb, two = _steps(hip, b, hip.to_device(b['T0']), 2)
    assert four[-1] > two[-1] > 0
    Ta = a['st'].run(hip.to_device(a['T0']), 2)
    assert a['st'].captures == 1 and _bits(np.asarray(Ta), np.asarray(Tb))
    _same_state(a, b, 'after two steps')
    # a run of no steps at all changes nothing
    before = a['mm'].ids
    a['st'].run(Ta, 0)
    assert np.array_equal(a['mm'].ids, before) and a['tr'].changed == two[-1]


# ---- 5. with every other part of the step -----------------------------------------------------------------------------------------
def test_the_step_with_loss_phase_the_recorders_and_a_monitor(hip, monkeypatch):
    r = tc.RULES['chain']
    prm = hip.Params(_dt(), 0.5)
    losses = (hip.SurfaceLoss(h=30.0, emissivity=0.4), hip.SurfaceLoss(h=80.0), hip.SurfaceLoss(h=10.0, emissivity=0.8),
              hip.SurfaceLoss(h=55.0, emissivity=0.2))
    regions = [((0, 20), (0, 18), (0, 35)), ((0, 16), (0, 16), (0, 16))]

    def rig(ids=None, f=None, T=None):
        c, grid, mm, mph, tr = _rig(hip, monkeypatch, 'odd', r, True, loss=True, ids=ids, f=f)
        T = hip.to_device(c['T'] if T is None else T)
        kw = dict(material_map=mm, surface_loss=hip.MapLossPacks(mm, losses, tc.TINF), phase=mph, transitions=tr,
                  history=hip.ThermalHistory(grid, hip.HistoryLevels(800.0, 500.0, 1400.0), capacity=8, T=T),
                  solidification=hip.SolidificationRecord(grid, 1400.0, T=T),
                  monitor=hip.FieldMonitor(grid, regions=regions, capacity=8, material_map=mm))
        return c, grid, mm, mph, tr, T, kw
    c, grid, mm, mph, tr, T, kw = rig()
    T1 = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, tc.TINF, **kw)
    n1 = tr.changed
    ids1, f1 = mm.ids, np.asarray(mph.liquid_fraction)
    assert n1 > 50 and (ids1 != c['ids']).sum() == n1
    # the monitor's heat content is weighed with the ids the step left
    w = FieldMonitor.weights_of(mm.materials, tc.DX)
    want = FieldMonitor.record_reference(np.asarray(T1), c['mask'], [], regions, weights=w, ids=ids1)['sum_wT']
    old = FieldMonitor.record_reference(np.asarray(T1), c['mask'], [], regions, weights=w, ids=c['ids'])['sum_wT']
    got = kw['monitor'].region_log()['heat'][:, 0]
    assert _bits(got, want) and not _bits(want, old)
    # the coefficient arrays of a changed cell are the zeros of the robin_h=None build until the next loss update; every other
    # cell keeps what this step's update wrote from its input, the flux arrays are those of the new ids
    changed = ids1 != c['ids']
    co = MapLossPacks.coeff_reference(c['T'], c['mask'], c['ids'], tc.MATERIALS, tc.DX, losses, tc.TINF)
    ref = MaterialMap.packs_reference(c['mask'], ids1, tc.MATERIALS, tc.DX, **tc.bc_of(c, True))
    for a in range(3):
        assert _bits(grid.layout.to_host(mm.packs[a].d_coeff), np.where(changed, 0.0, co[a])), a
        assert _bits(grid.layout.to_host(mm.packs[a].d_qflux), ref[a].qflux), a
    assert any((co[a][changed] != 0.0).any() for a in range(3))
    # the step after the transition is the step of a rig built anew around the same (T, f, ids)
    T2 = hip.adi_step_numba_coeff(T1, grid, mm.mat, prm, mm.packs, tc.TINF, **kw)
    c, grid_n, mm_n, mph_n, tr_n, Tn, kw_n = rig(ids=ids1, f=f1, T=np.asarray(T1))
    T2n = hip.adi_step_numba_coeff(Tn, grid_n, mm_n.mat, prm, mm_n.packs, tc.TINF, **kw_n)
    assert _bits(np.asarray(T2), np.asarray(T2n)) and not _bits(np.asarray(T2), np.asarray(T1))
    assert np.array_equal(mm.ids, mm_n.ids) and _bits(np.asarray(mph.liquid_fraction), np.asarray(mph_n.liquid_fraction))
    assert tr.changed - n1 == tr_n.changed > 0               # (the chain's second hop, at the least)
    assert torch.equal(tr.brick_ids, tr_n.brick_ids) and torch.equal(mph.summary, mph_n.summary)


# ---- 6. freshness --------------------------------------------------------------------------------------------------------------
def test_a_stale_object_raises_before_any_launch(hip, monkeypatch):
    r = tc.RULES['powder']
    c, grid, mm, mph, tr = _rig(hip, monkeypatch, 'odd', r, True)
    prm = hip.Params(_dt(), 0.5)
    T = hip.to_device(c['T'])
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, tc.TINF, material_map=mm, phase=mph, transitions=tr)
    mask2 = np.array(c['mask'])
    mask2[:, :, 30:] = False
    grid.mask = mask2
    mm.rebuild()
    mph.sync_mask(T)
    launched = []
    monkeypatch.setattr(mm, '_explicit_into', lambda *a: launched.append(a))
    for call in (lambda: st.step(T), lambda: st.run(T, 2),
                 lambda: hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, tc.TINF, material_map=mm, phase=mph, transitions=tr),
                 lambda: tr.apply(T)):
        with pytest.raises(ValueError, match=r'MaterialTransitions: .*sync_mask\(\)'):
            call()
    assert not launched and tr.changed == 0 and np.array_equal(mm.ids, c['ids'])
    monkeypatch.undo()
    tr.sync_mask()
    T1 = st.step(T)
    ids1, f1, n1 = tc.reference(r, np.asarray(T1), None, mask2, c['ids'], c['dir_mask'])
    assert tr.changed == n1 > 0 and np.array_equal(mm.ids, ids1)
    # new ids: stale again, and with a phase the phase's sync comes first
    mm.set_ids(np.array(c['ids']))
    with pytest.raises(ValueError, match='sync_mask'):
        tr.sync_mask()
    mph.sync_mask(T)
    with pytest.raises(ValueError, match=r'MaterialTransitions: .*sync_mask\(\)'):
        st.step(T)
    tr.sync_mask()
    st.step(T)
    # what the step refuses on the device as on the host
    with pytest.raises(ValueError, match='needs material_map='):
        hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, tc.TINF, transitions=tr)
    with pytest.raises(ValueError, match="is not the step's phase="):
        hip.StagedStepper(grid, mm.mat, prm, mm.packs, tc.TINF, material_map=mm, transitions=tr)
    assert isinstance(tr, MaterialTransitions)
