"""GPU: the Cartesian step on a grid of several materials (MaterialMap, material_map=) against its definition
(MaterialMap.packs_reference / step_reference, NumPy fp64) and the extended-precision reference tests/matmap_ref_ld.py.  Cases,
metric and bar: tests/matmap_cases.py.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import matmap_cases as mc
import matmap_ref_ld

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def _setup(hip, c, ids=None, mask=None):
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'] if mask is None else mask)
    mm = hip.MaterialMap(grid, c['materials'], np.array(c['ids'] if ids is None else ids), **mc.bc_of(c))
    return grid, mm, hip.Params(c['dt'], c['theta'])


def _step(hip, c, T0=None, S=None, **kw):
    grid, mm, prm = _setup(hip, c, **kw)
    return hip.adi_step_numba_coeff(np.array(c['T0'] if T0 is None else T0), grid, mm.mat, prm, mm.packs, c['Tinf'],
                                    material_map=mm, S=S)


def _hold(X, c, ref, what, a=None):
    X = np.asarray(X)
    assert np.all(np.isfinite(X)), what
    ok, f = mc.meets_bar(X, c, ref, a)
    print('%-80s inc %.2e K  err %.2e K = %8.2f ulp = %.1e inc  bar %.2e' % (what, f['inc'], f['abs_err'], f['ulp'], f['of_inc'],
                                                                           mc.bar(f, mc.A_MAP if a is None else a)))
    assert mc.untouched_exact(X, c), what
    assert ok, (what, f)


def _definition(c, **kw):
    from adi_thermal_fields_amd.packs import MaterialMap
    return mc.run(MaterialMap.step_reference, MaterialMap.packs_reference, c, **kw)


HOLES_KEY = ('holes', mc.HOLES, 'random3', 'general', 0.5, 200.0)


# ---- 1. packs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['scalar', 'dict', 'voxel', 'flux_array_dirichlet'])
def test_packs_bit_equal_to_the_definition(hip, form):
    c = mc.case(HOLES_KEY)
    rng = np.random.default_rng(11)
    bc = dict(dir_mask=None, dir_value=None, neumann=None, robin_h=None)
    if form == 'scalar':
        bc.update(robin_h=350.0, neumann={'z-': 2e5})
    elif form == 'dict':
        bc.update(robin_h={'x-': 410.0, 'x+': 37.5, 'y+': 999.0, 'z-': 12.25}, neumann={'x+': 2e5, 'z-': -3.5e4})
    elif form == 'voxel':
        bc.update(robin_h=rng.uniform(20.0, 400.0, c['shape']))
    else:
        bc = mc.bc_of(c)
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    mm = hip.MaterialMap(grid, c['materials'], np.array(c['ids']), **bc)
    want = hip.MaterialMap.packs_reference(c['mask'], c['ids'], c['materials'], c['dx'], **bc)
    assert all(p.face_consts is None and p.sparse_ok for p in mm.packs)
    for a in range(3):
        assert np.array_equal(mm.packs[a].coeff, want[a].coeff), (form, a)
        assert np.array_equal(mm.packs[a].qflux, want[a].qflux), (form, a)
        assert np.array_equal(mm.packs[a].dir_mask, want[a].dir_mask), (form, a)
        if bc['dir_mask'] is not None:
            assert np.array_equal(mm.packs[a].dir_val, want[a].dir_val), (form, a)
    assert np.any(want[0].coeff != 0) and np.array_equal(mm.ids, c['ids'])


# ---- 2. stages --------------------------------------------------------------------------------------------------------------
def test_each_stage_against_the_definitions_stage_from_the_same_input(hip):
    c = mc.case(HOLES_KEY)
    grid, mm, prm = _setup(hip, c)
    _, st64 = _definition(c, return_stages=True)
    mask = c['mask']
    idm = np.where(mask, c['ids'], 0).astype(np.intp)
    pk = matmap_ref_ld.packs(mask, c['ids'], c['materials'], c['dx'], **mc.bc_of(c))
    G = matmap_ref_ld.pair_table(c['materials'], c['dx'], c['dt'])
    LD = np.longdouble
    # R0 from T0
    got = mm.explicit_rhs(np.array(c['T0']), prm)
    want = matmap_ref_ld.explicit(c['T0'], mask, idm, G, 1 - LD(c['theta']))
    _hold_stage(got, want, c['T0'], c, 'R0')
    print('R0 bit-equal to the fp64 definition: %s' % np.array_equal(got, st64['R0']))
    # U, V, W each from the definition's fp64 input of that stage
    for axis, (src, name) in enumerate((('R0', 'U'), ('U', 'V'), ('V', 'W'))):
        X = np.array(st64[src])
        got = mm.sweep_axis(axis, X, prm, c['Tinf'])
        want = matmap_ref_ld.sweep(axis, X.astype(LD), mask, idm, LD(c['theta']) * G, c['dt'], pk[axis], c['Tinf'])
        _hold_stage(got, want, X, c, name)


def _hold_stage(got, want, X0, c, name):
    """the bar of one step applied to one stage: its own input X0 in place of T0"""
    mask = c['mask']
    dirc = mask & c['dir_mask']
    free = mask & ~dirc
    err = float(np.max(np.abs(got - want)[mask]))
    inc = float(np.max(np.abs(want - X0)[free]))
    wmax = float(np.max(np.abs(want[mask])))
    b = mc.A_MAP * mc.EPS64 * wmax + 1e-10 * inc
    print('stage %-3s err %.2e = %.2f ulp, inc %.2e, bar %.2e' % (name, err, err / (mc.EPS64 * wmax), inc, b))
    assert np.array_equal(got[~mask], X0[~mask]), name
    if name != 'R0':
        assert np.array_equal(got[dirc], c['dir_value'][dirc]), name
    assert err <= b, (name, err, b)


# ---- 3. one step against the long-double reference --------------------------------------------------------------------------
@pytest.mark.parametrize(**mc.params(lambda k: k[0] == 'holes'))
def test_one_step_holes_padded(hip, monkeypatch, key):
    monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx + 1, ny + 2, nz + 3))
    c = mc.case(key)
    grid, mm, prm = _setup(hip, c)
    assert grid.layout.padded
    X = hip.adi_step_numba_coeff(np.array(c['T0']), grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
    _hold(X, c, mc.reference(key), mc.tag(key))


@pytest.mark.parametrize(**mc.params(lambda k: k[0] in ('layers', 'long', 'past_limit', 'rows16')))
def test_one_step(hip, key):
    c = mc.case(key)
    _hold(_step(hip, c), c, mc.reference(key), mc.tag(key))


def test_ids_of_255_off_the_mask_change_nothing(hip):
    c = mc.case(HOLES_KEY)
    ids = np.array(c['ids'])
    ids[~c['mask']] = 255
    assert np.array_equal(_step(hip, c), _step(hip, c, ids=ids))


# ---- 4. all ids 0 -----------------------------------------------------------------------------------------------------------
def test_all_ids_zero_is_the_plain_material(hip):
    import cart_ref_ld
    from helpers import run_cart_case
    key = ('holes', mc.HOLES, 'zero', 'general', 0.5, 200.0)
    c = mc.case(key)
    rho, cp, k = c['materials'][0]
    cc = dict(shape=c['shape'], dx=c['dx'], mat=dict(rho=rho, cp=cp, k=k), mask=c['mask'], T0=c['T0'], dt=c['dt'], theta=c['theta'],
              Tinf=c['Tinf'], nsteps=1, births=None, **mc.bc_of(c))
    W = run_cart_case(cart_ref_ld, cc)['T_final']
    ref = (W[c['mask']], float(np.max(np.abs(W - c['T0'])[c['mask'] & ~c['dir_mask']])), float(np.max(np.abs(W[c['mask']]))))
    X = _step(hip, c)
    _hold(X, c, ref, 'ids 0 vs the plain reference')
    plain = run_cart_case(hip, cc)['T_final']
    f = mc.figures_of(X, c, ref)
    d = float(np.max(np.abs(X - plain)[c['mask']]))
    print('ids 0 vs the plain HIP step: %.2e, twice the bar %.2e' % (d, 2 * mc.bar(f, mc.A_MAP)))
    assert d <= 2 * mc.bar(f, mc.A_MAP)


# ---- 5. StagedStepper -------------------------------------------------------------------------------------------------------
def test_staged_stepper_step_run_graph_and_a_new_dt(hip):
    key = ('holes', mc.HOLES, 'random3', 'general', 1.0, 200.0)
    c = mc.case(key)
    grid, mm, prm = _setup(hip, c)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
    assert not st.fused and len(st.stage_names) == 4
    _hold(st.step(hip.to_device(c['T0'])).get(), c, mc.reference(key), 'StagedStepper.step')
    T = hip.to_device(c['T0'])
    for _ in range(6):
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
    six = T.get()
    got = st.run(hip.to_device(c['T0']), 6).get()
    assert st.captures == 1 and np.array_equal(got, six)
    assert np.array_equal(st.run(hip.to_device(c['T0']), 6, graph=False).get(), six)
    # a new dt: the next run recaptures, and its first two steps (one replay) are those of the new table
    prm.dt = 0.37 * c['dt']
    c2 = dict(c, dt=prm.dt)
    two = st.run(hip.to_device(c['T0']), 2).get()
    assert st.captures == 2
    W1 = mc.run(matmap_ref_ld.step, matmap_ref_ld.packs, c2)
    T1 = np.asarray(hip.adi_step_numba_coeff(np.array(c['T0']), grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm))
    _hold(T1, c2, mc.reference_of(c2), 'one step at the new dt')
    _hold(two, c2, mc.reference_of(c2, T0=T1), 'graph replay at the new dt, second step from the first', )
    assert not np.array_equal(W1[c['mask']].astype(np.float64), mc.reference(key)[0].astype(np.float64))


# ---- 6. source field --------------------------------------------------------------------------------------------------------
def test_source_field_as_array_and_sampled_on_the_device(hip):
    key = ('holes', mc.HOLES, 'random3', 'general', 0.5, 0.3)
    c = mc.case(key)
    rng = np.random.default_rng(5)
    S = rng.uniform(0.0, 5e10, c['shape'])
    _hold(_step(hip, c, S=S), c, mc.reference_of(c, S=S), 'S as a NumPy array')
    assert not np.array_equal(mc.reference_of(c, S=S)[0], mc.reference(key)[0])
    grid, mm, prm = _setup(hip, c)
    path = hip.ScanPath(eta=0.8, a=3e-3, b=3e-3, c_f=3e-3, c_r=6e-3, power=2000.0, start=(5e-3, 9e-3, 35e-3))
    path.line_to((15e-3, 9e-3, 35e-3), speed=0.01)
    d_S = path.on_device().sample_step_device(grid, 0.0, c['dt'])
    Sh = np.asarray(d_S)
    assert Sh.max() > 0.0
    X = hip.adi_step_numba_coeff(np.array(c['T0']), grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=d_S)
    _hold(X, c, mc.reference_of(c, S=Sh), 'S from sample_step_device')


# ---- 7. birth ---------------------------------------------------------------------------------------------------------------
def test_birth_across_a_material_interface_then_rebuild(hip):
    key = ('layers', mc.LAYERS, ('layers', 2, 16), 'robin_neumann', 1.0, 200.0)
    c = mc.case(key)
    full = np.array(c['mask'])
    first = full.copy(); first[:, :, 15:] = False          # planes 15 and 16 are born: one either side of the interface
    second = full.copy(); second[:, :, 17:] = False
    grid, mm, prm = _setup(hip, c, mask=first)
    from adi_thermal_fields_amd.packs import MaterialMap
    T = np.array(c['T0']); Tdef = np.array(c['T0'])
    for n, mask in enumerate((first, second)):
        if n:
            newborn = mask & ~first
            T[newborn] = 1400.0; Tdef[newborn] = 1400.0
            grid.mask = mask
            with pytest.raises(ValueError, match='rebuild'):
                hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
            mm.rebuild()
        want = MaterialMap.packs_reference(mask, c['ids'], c['materials'], c['dx'], **mc.bc_of(c))
        for a in range(3):
            assert np.array_equal(mm.packs[a].coeff, want[a].coeff) and np.array_equal(mm.packs[a].qflux, want[a].qflux), (n, a)
        cn = dict(c, mask=mask)
        for s in range(3):
            ref = mc.reference_of(cn, T0=T)
            Tdef = MaterialMap.step_reference(T, mask, c['ids'], c['materials'], c['dx'], c['dt'], c['theta'], want, c['Tinf'])
            Tn = np.asarray(hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm))
            _hold(Tn, dict(cn, T0=T), ref, 'birth phase %d step %d' % (n, s))
            _hold(Tdef, dict(cn, T0=T), ref, 'birth phase %d step %d, definition' % (n, s))
            T = Tn


# ---- 8. recorders -----------------------------------------------------------------------------------------------------------
def test_history_and_solidification_with_a_material_map(hip):
    key = ('holes', mc.HOLES, 'random3', 'general', 1.0, 0.3)
    c = mc.case(key)
    grid, mm, prm = _setup(hip, c)
    lv = hip.HistoryLevels(800.0, 500.0, 1400.0)
    T_freeze = 1000.0
    T0 = hip.to_device(c['T0'])
    hist = hip.ThermalHistory(grid, lv, T=T0)
    rec = hip.SolidificationRecord(grid, T_freeze, T=T0)
    nan3 = lambda: tuple(np.full(c['shape'], np.nan) for _ in range(3))
    hs = hip.ThermalHistory.seed_reference(nan3(), c['T0'], c['mask'])
    rs = hip.SolidificationRecord.seed_reference(nan3(), c['T0'], c['mask'])
    T, t = T0, 0.0
    frozen = 0
    for _ in range(3):
        Tn = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, history=hist, solidification=rec)
        A, B = np.asarray(T), np.asarray(Tn)
        hs, _ = hip.ThermalHistory.record_reference(hs, A, B, c['mask'], t, prm.dt, lv)
        rs = hip.SolidificationRecord.record_reference(rs, A, B, c['mask'], t, prm.dt, c['dx'], T_freeze)
        frozen += int((c['mask'] & (A > T_freeze) & (B <= T_freeze)).sum())
        T, t = Tn, t + prm.dt
    assert frozen > 0
    for name, got, w in zip(('T_peak', 't_hi', 't_lo'), (hist.T_peak, hist.t_hi, hist.t_lo), hs):
        assert np.array_equal(np.asarray(got), w, equal_nan=True), name
    for name, got, w in zip(('t_solid', 'cooling_rate', 'g2'), (rec.t_solid, rec.cooling_rate, rec.g2), rs):
        assert np.array_equal(np.asarray(got), w, equal_nan=True), name


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refused_combinations_raise_before_any_launch(hip):
    c = mc.case(HOLES_KEY)
    grid, mm, prm = _setup(hip, c)
    grid2, mm2, _ = _setup(hip, c)
    T = hip.to_device(c['T0'])
    before = T.get()
    step = lambda *a, **kw: hip.adi_step_numba_coeff(T, *a, **kw)
    src = hip.GoldakSource(power=2000.0, eta=0.8, a=3e-3, b=3e-3, c_f=3e-3, c_r=6e-3, origin=(5e-3, 9e-3, 34e-3),
                           velocity=0.01, travel_axis=0, depth_axis=2)
    other = hip.precompute_coeff_packs_unified(grid, mm.mat, robin_h=350.0)
    with pytest.raises(ValueError, match='GoldakSource'):
        step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=src)
    with pytest.raises(ValueError, match='own packs'):
        step(grid, mm.mat, prm, other, c['Tinf'], material_map=mm)
    with pytest.raises(ValueError, match='own material'):
        step(grid, hip.Material(*mc.COPPER), prm, mm.packs, c['Tinf'], material_map=mm)
    with pytest.raises(ValueError, match='another grid'):
        step(grid, mm2.mat, prm, mm2.packs, c['Tinf'], material_map=mm2)
    with pytest.raises(TypeError, match='MaterialMap'):
        step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=object())
    for kw in ('surface_loss', 'material'):
        with pytest.raises(ValueError, match='one cp'):
            step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, **{kw: object()})
    phase = hip.PhaseField(grid, hip.Material(*mc.STEEL), hip.PhaseChange(2.7e5, 1400.0, 1450.0), T=T)
    with pytest.raises(ValueError, match='one cp'):
        step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, phase=phase)
    with pytest.raises(ValueError, match='GoldakSource'):
        hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, source=src)
    assert np.array_equal(T.get(), before)
