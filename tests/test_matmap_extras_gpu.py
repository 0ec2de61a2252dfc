"""GPU: latent heat and surface loss with one law per material of a MaterialMap (MapPhaseField, MapLossPacks).  The
two pointwise kernels against their definitions bit for bit on the same inputs, the step with them against the extended-precision
reference (the bar A_MAP of tests/matmap_cases.py) and against the definition of the correction, StagedStepper's graph against
plain launches, the enthalpy of an adiabatic body, and what is refused.  Laws, fields and the coverage condition:
tests/matmap_extras_cases.py.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import matmap_cases as mc
import matmap_extras_cases as xc
from adi_thermal_fields_amd.packs import _nbr_in_mask

pytestmark = pytest.mark.gpu

HOLES_KEY = ('holes', mc.HOLES, 'random3', 'general', 0.5, 200.0)
LAYERS_KEY = ('layers', mc.LAYERS, ('layers', 0, 17), 'robin_neumann', 0.5, 200.0)
GRIDS = ['holes', 'holes_padded', 'layers15', 'layers16', 'layers17', 'shells', 'bricks35', 'special']


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _grid_case(name):
    """dict(shape, mask, ids, materials, nan) of a pointwise case; nan: cells whose T no kernel may read (None: none)"""
    if name in ('holes', 'holes_padded'):
        c = mc.case(HOLES_KEY)
    elif name.startswith('layers'):
        c = mc.case(('layers', mc.LAYERS, ('layers', 0, int(name[6:])), 'robin_neumann', 0.5, 200.0))
    elif name == 'shells':
        c = mc.case(('long', (40, 33, 50), 'shells3', 'general', 0.5, 0.3))
    elif name == 'bricks35':
        c = mc.case(('long', (8, 16, 560), 'shells3', 'general', 0.5, 0.3))
    else:
        # brick (0, 0, 0) wholly insulator (no law), brick (0, 0, 1) without an in-mask cell, the rest mixed with holes
        shape = (32, 16, 48)
        rng = np.random.default_rng(17)
        mask = rng.random(shape) > 0.25
        ids = rng.integers(0, 3, shape).astype(np.uint8)
        mask[:16, :, :16] = True
        ids[:16, :, :16] = 2
        mask[:16, :, 16:32] = False
        nan = np.zeros(shape, bool)
        nan[:16, :, :32] = True
        return dict(shape=shape, mask=mask, ids=ids, materials=mc.MATERIALS, nan=nan)
    return dict(shape=c['shape'], mask=c['mask'], ids=np.array(c['ids']), materials=c['materials'], nan=None)


def _build(hip, monkeypatch, name, **bc):
    if name == 'holes_padded':
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx + 1, ny + 2, nz + 3))
    g = _grid_case(name)
    grid = hip.Grid3D(*g['shape'], mc.DX, g['mask'])
    assert grid.layout.padded or name != 'holes_padded'
    mm = hip.MaterialMap(grid, g['materials'], g['ids'], **bc)
    return g, grid, mm


def _words(t):
    return t.cpu().numpy()


# ---- 1. seed and apply, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GRIDS)
def test_seed_and_apply_bit_equal_to_the_definition(hip, monkeypatch, name):
    g, grid, mm = _build(hip, monkeypatch, name)
    mask, ids, mats = g['mask'], g['ids'], g['materials']
    laws = xc.laws_of(mats)
    fl = xc.fields(mask, ids, laws)
    xc.assert_covered(fl['T_star'], fl['f0'], mask, ids, fl['dir_mask'], mats, name)       # (on the CPU, before any launch)
    T_seed, T_star = np.array(fl['T_seed']), np.array(fl['T_star'])
    if g['nan'] is not None:
        T_seed[g['nan']] = np.nan
        T_star[g['nan']] = np.nan
    pd = grid.layout.pd[:3]
    want_ids = xc.brick_words(mask, ids, pd)
    if name == 'layers16':
        assert set(want_ids.tolist()) <= {1, 2} and {1, 2} <= set(want_ids.tolist())      # uniform bricks only
    if name in ('layers15', 'layers17', 'holes'):
        assert any(bin(w).count('1') > 1 for w in want_ids.tolist())
    if name == 'special':
        assert want_ids[0] == 4 and want_ids[1] == 0
    # seed
    mph = hip.MapPhaseField(mm, laws, T=hip.to_device(T_seed))
    f0 = xc.MapPhaseField.f_eq_of(laws, T_seed, mask, ids)
    assert _bits(f0, fl['f0'])
    assert _bits(np.asarray(mph.liquid_fraction), f0), name
    assert np.array_equal(_words(mph.summary), xc.brick_any(f0, pd)), name
    assert np.array_equal(_words(mph.brick_ids), want_ids), name
    # apply
    T = hip.to_device(T_star)
    dm = grid.layout.to_layout(fl['dir_mask'], torch.uint8)
    mph.apply(T, dm)
    want_T, want_f = xc.MapPhaseField.correct_of(laws, mats, T_star, f0, mask, ids, fl['dir_mask'])
    assert _bits(mph.correct(T_star, f0, mask, ids, fl['dir_mask'])[0], want_T)
    got_T, got_f = np.asarray(T), np.asarray(mph.liquid_fraction)
    assert _bits(got_T, want_T), (name, int((got_T.view(np.uint64) != want_T.view(np.uint64)).sum()))
    assert _bits(got_f, want_f), (name, int((got_f != want_f).sum()))
    assert np.array_equal(_words(mph.summary), xc.brick_any(want_f, pd)), name
    assert np.array_equal(_words(mph.brick_ids), want_ids), name
    assert not _bits(want_T, T_star) and not _bits(want_f, f0)
    # a second pass from the state the first left, without Dirichlet cells
    mph.apply(T)
    want_T2, want_f2 = xc.MapPhaseField.correct_of(laws, mats, want_T, want_f, mask, ids, None)
    assert _bits(np.asarray(T), want_T2) and _bits(np.asarray(mph.liquid_fraction), want_f2), name
    assert np.array_equal(_words(mph.summary), xc.brick_any(want_f2, pd)), name


def test_seed_selection_set_liquid_fraction_snapshot_and_sync(hip, monkeypatch):
    g, grid, mm = _build(hip, monkeypatch, 'holes')
    mask, ids, mats = g['mask'], g['ids'], g['materials']
    laws = xc.laws_of(mats)
    fl = xc.fields(mask, ids, laws)
    pd = grid.layout.pd[:3]
    mph = hip.MapPhaseField(mm, laws)                                 # no T: all solid, brick_ids built
    assert not np.asarray(mph.liquid_fraction).any() and not _words(mph.summary).any()
    assert np.array_equal(_words(mph.brick_ids), xc.brick_words(mask, ids, pd))
    mph.seed(hip.to_device(fl['T_seed']))
    snap = mph.snapshot()
    # a seed of selected cells from another field: they take f_eq of their own law, the others keep f
    rng = np.random.default_rng(23)
    sel = rng.random(mask.shape) < 0.3
    other = xc.MapPhaseField.f_eq_of(laws, fl['T_star'], mask, ids)
    mph.seed(hip.to_device(fl['T_star']), sel=sel)
    want = np.where(sel, other, fl['f0'])
    assert _bits(np.asarray(mph.liquid_fraction), want)
    assert np.array_equal(_words(mph.summary), xc.brick_any(want, pd))
    mph.restore(snap)
    assert _bits(np.asarray(mph.liquid_fraction), fl['f0']) and np.array_equal(_words(mph.summary), xc.brick_any(fl['f0'], pd))
    # a loaded f: taken as 0 off the mask and where the material has no law
    load = rng.uniform(0.0, 1.0, mask.shape)
    mph.set_liquid_fraction(load)
    want = np.where(mask & (ids != 2), load, 0.0)
    assert _bits(np.asarray(mph.liquid_fraction), want) and np.array_equal(_words(mph.summary), xc.brick_any(want, pd))
    # new ids: stale until sync_mask, which rebuilds brick_ids (and clears f where the material has no law now)
    ids2 = np.roll(ids, 5, axis=2)
    mm.set_ids(ids2)
    T = hip.to_device(fl['T_star'])
    with pytest.raises(ValueError, match='sync_mask'):
        mph.apply(T)
    mph.sync_mask(T)
    assert np.array_equal(_words(mph.brick_ids), xc.brick_words(mask, ids2, pd))
    want = np.where(ids2 != 2, want, 0.0)
    assert _bits(np.asarray(mph.liquid_fraction), want)
    # a new mask: the cells that joined are seeded from T, those that left cleared
    mask2 = mask.copy()
    mask2[:, :, 30:] = ~mask[:, :, 30:]
    grid.mask = mask2
    with pytest.raises(ValueError, match='sync_mask'):
        mph.apply(T)
    mph.sync_mask(T)
    joined = mask2 & ~mask
    want = np.where(joined, xc.MapPhaseField.f_eq_of(laws, fl['T_star'], mask2, ids2), np.where(mask2, want, 0.0))
    assert _bits(np.asarray(mph.liquid_fraction), want)
    assert np.array_equal(_words(mph.brick_ids), xc.brick_words(mask2, ids2, pd))
    assert np.array_equal(_words(mph.summary), xc.brick_any(want, pd))
    mm.rebuild()
    mph.apply(T)


# ---- 2. update and rebuild, bit for bit ------------------------------------------------------------------------------------------
def _exposed(mask, axis):
    return mask & ~(_nbr_in_mask(mask, axis, False) & _nbr_in_mask(mask, axis, True))


SENTINEL = -7.0


@pytest.mark.parametrize('name', GRIDS)
def test_update_and_rebuild_bit_equal_to_the_definition(hip, monkeypatch, name):
    g, grid, mm = _build(hip, monkeypatch, name)
    mask, ids, mats = g['mask'], g['ids'], g['materials']
    losses = xc.losses_of(mats)
    rng = np.random.default_rng(31)
    T = rng.uniform(100.0, 1900.0, g['shape'])              # below the first knot of the table and beyond its last
    Td = hip.to_device(T)
    lp = hip.MapLossPacks(mm, losses, xc.TINF)
    assert lp.packs is mm.packs
    for a in range(3):
        assert not mm.packs[a].coeff.any()
        mm.packs[a].d_coeff.fill_(SENTINEL)
    lp.update(Td)
    want = hip.MapLossPacks.coeff_reference(T, mask, ids, mats, mc.DX, losses, xc.TINF)
    for a in range(3):
        got, ex = mm.packs[a].coeff, _exposed(mask, a)
        assert ex.any() and (want[a][ex] > 0.0).all()
        assert _bits(got[ex], want[a][ex]), (name, a, int((got[ex] != want[a][ex]).sum()))
        assert (got[~ex] == SENTINEL).all(), (name, a)       # update leaves the cells that are not exposed alone
    # a new ambient in the call
    lp.update(Td, Tinf=35.0)
    want35 = hip.MapLossPacks.coeff_reference(T, mask, ids, mats, mc.DX, losses, 35.0)
    for a in range(3):
        got, ex = mm.packs[a].coeff, _exposed(mask, a)
        assert _bits(got[ex], want35[a][ex]) and not _bits(want35[a][ex], want[a][ex]), (name, a)
    # rebuild: a plane range in full, zeros where a cell is not exposed, nothing outside the range
    k0, k1 = 5, min(21, g['shape'][2] - 2)
    for a in range(3):
        mm.packs[a].d_coeff.fill_(SENTINEL)
    lp.rebuild(Td, k0, k1)
    for a in range(3):
        got = mm.packs[a].coeff
        assert _bits(got[:, :, k0:k1], want[a][:, :, k0:k1]), (name, a)
        assert (got[:, :, :k0] == SENTINEL).all() and (got[:, :, k1:] == SENTINEL).all(), (name, a)
    lp.rebuild(Td)
    for a in range(3):
        assert _bits(mm.packs[a].coeff, want[a]), (name, a)
    # T (here): evaluated at once
    mm2 = hip.MaterialMap(grid, mats, ids)
    hip.MapLossPacks(mm2, losses, xc.TINF, T=Td)
    for a in range(3):
        assert _bits(mm2.packs[a].coeff, want[a]), (name, a)


def test_after_a_birth_and_the_maps_rebuild_an_update_is_enough(hip):
    """a stale MapLossPacks is not an error: mm.rebuild() leaves zeros (no h was given) and update writes every exposed cell"""
    c = mc.case(('layers', mc.LAYERS, ('layers', 2, 16), 'robin_neumann', 1.0, 200.0))
    full = np.array(c['mask'])
    first = full.copy(); first[:, :, 15:] = False
    second = full.copy(); second[:, :, 17:] = False
    ids, mats = np.array(c['ids']), c['materials']
    losses = xc.losses_of(mats)
    grid = hip.Grid3D(*c['shape'], mc.DX, first)
    mm = hip.MaterialMap(grid, mats, ids, neumann=c['neumann'])
    lp = hip.MapLossPacks(mm, losses, xc.TINF)
    rng = np.random.default_rng(37)
    T = rng.uniform(100.0, 1900.0, c['shape'])
    Td = hip.to_device(T)
    lp.update(Td)
    for mask in (first, second):
        if mask is second:
            grid.mask = second
            mm.rebuild()
            lp.update(Td)
        want = hip.MapLossPacks.coeff_reference(T, mask, ids, mats, mc.DX, losses, xc.TINF)
        for a in range(3):
            assert _bits(mm.packs[a].coeff, want[a]), a
    assert not _bits(want[2], hip.MapLossPacks.coeff_reference(T, first, ids, mats, mc.DX, losses, xc.TINF)[2])


# ---- 3. the step -----------------------------------------------------------------------------------------------------------------
def _step_case(hip, key):
    c = mc.case(key)
    bc = dict(mc.bc_of(c), robin_h=None)
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    ids, mats = np.array(c['ids']), c['materials']
    mm = hip.MaterialMap(grid, mats, ids, **bc)
    laws, losses = xc.laws_of(mats), xc.losses_of(mats)
    fl = xc.fields(c['mask'], ids, laws, seed=1)
    T0 = np.array(fl['T_star'])
    lp = hip.MapLossPacks(mm, losses, c['Tinf'])
    return c, grid, mm, hip.Params(c['dt'], c['theta']), laws, losses, fl, T0, lp


@pytest.mark.parametrize('key', [HOLES_KEY, LAYERS_KEY], ids=[mc.tag(HOLES_KEY), mc.tag(LAYERS_KEY)])
def test_one_step_with_loss_then_with_latent_heat(hip, key):
    c, grid, mm, prm, laws, losses, fl, T0, lp = _step_case(hip, key)
    mask, ids, mats = c['mask'], np.array(c['ids']), c['materials']
    # X: surface_loss= alone, against the long-double step whose packs hold the per-cell h_of fields
    X = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp))
    cr = dict(c, T0=T0, robin_h=xc.h_fields(T0, mask, ids, mats, c['Tinf']))
    ref = mc.reference_of(cr)
    ok, f = mc.meets_bar(X, cr, ref)
    print('%-70s inc %.2e K  err %.2e K = %8.2f ulp  bar %.2e' % (mc.tag(key), f['inc'], f['abs_err'], f['ulp'], mc.bar(f, mc.A_MAP)))
    assert np.all(np.isfinite(X)) and mc.untouched_exact(X, cr) and ok, f
    plain = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm))
    assert _bits(plain, X)                                  # (the arrays stay as the update left them)
    # Y: phase= too, bit for bit the definition of the correction on X
    mph = hip.MapPhaseField(mm, laws, T=hip.to_device(fl['T_seed']))
    f0 = np.asarray(mph.liquid_fraction)
    assert _bits(f0, fl['f0'])
    Y = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp,
                                            phase=mph))
    want_Y, want_f = mph.correct(X, f0, mask, ids, c['dir_mask'])
    assert _bits(Y, want_Y) and _bits(np.asarray(mph.liquid_fraction), want_f)
    assert not _bits(Y, X) and not _bits(want_f, f0)
    # phase= alone
    mm0 = hip.MaterialMap(grid, mats, ids, **dict(mc.bc_of(c), robin_h=None))
    mph0 = hip.MapPhaseField(mm0, laws, T=hip.to_device(fl['T_seed']))
    X0 = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm0.mat, prm, mm0.packs, c['Tinf'], material_map=mm0))
    Y0 = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm0.mat, prm, mm0.packs, c['Tinf'], material_map=mm0, phase=mph0))
    want_Y0, want_f0 = mph0.correct(X0, f0, mask, ids, c['dir_mask'])
    assert _bits(Y0, want_Y0) and _bits(np.asarray(mph0.liquid_fraction), want_f0) and not _bits(X0, X)


# ---- 4. StagedStepper ------------------------------------------------------------------------------------------------------------
def _state(T, mph, mm):
    return [np.asarray(T), np.asarray(mph.liquid_fraction)] + [np.array(mm.packs[a].coeff) for a in range(3)]


def _same(a, b):
    return all(_bits(x, y) for x, y in zip(a, b))


def test_staged_stepper_step_run_graph_plain_calls_and_a_new_dt(hip):
    c, grid, mm, prm, laws, losses, fl, T0, lp = _step_case(hip, HOLES_KEY)
    mph = hip.MapPhaseField(mm, laws, T=hip.to_device(fl['T_seed']))
    snap = mph.snapshot()
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp, phase=mph)
    bare = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
    assert st.stage_names == bare.stage_names and not st.fused

    def three_ways():
        out = []
        mph.restore(snap)
        T = hip.to_device(T0)
        for _ in range(5):
            T = st.step(T)
        out.append(_state(T, mph, mm))
        mph.restore(snap)
        out.append(_state(st.run(hip.to_device(T0), 5), mph, mm))
        mph.restore(snap)
        T = hip.to_device(T0)
        for _ in range(5):
            T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp, phase=mph)
        out.append(_state(T, mph, mm))
        return out

    a, b, d = three_ways()
    assert st.captures == 1
    assert _same(a, b) and _same(a, d)
    assert not _bits(a[1], fl['f0']) and a[2].any()
    prm.dt = 0.37 * c['dt']
    a2, b2, d2 = three_ways()
    assert st.captures == 2
    assert _same(a2, b2) and _same(a2, d2) and not _bits(a2[0], a[0])


def test_graph_with_history_solidification_and_a_monitor_of_f(hip):
    c, grid, mm, prm, laws, losses, fl, T0, lp = _step_case(hip, HOLES_KEY)
    mask, ids, mats = c['mask'], np.array(c['ids']), c['materials']
    mph = hip.MapPhaseField(mm, laws, T=hip.to_device(fl['T_seed']))
    snap = mph.snapshot()
    # five plain steps: the fields the monitor's definition is evaluated from
    T = hip.to_device(T0)
    states = []
    for _ in range(5):
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp, phase=mph)
        states.append((np.asarray(T), np.asarray(mph.liquid_fraction)))
    mph.restore(snap)
    T0d = hip.to_device(T0)
    regions = (None, ((2, 19), (0, 18), (3, 30)))
    probes = ((3, 4, 5), (10, 9, 20))
    mon = hip.FieldMonitor(grid, probes=probes, regions=regions, capacity=8, material_map=mm, extra=mph.f)
    hist = hip.ThermalHistory(grid, hip.HistoryLevels(800.0, 500.0, 1400.0), T=T0d)
    rec = hip.SolidificationRecord(grid, 1000.0, T=T0d)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp, phase=mph, history=hist,
                           solidification=rec, monitor=mon)
    out = st.run(T0d, 5)
    assert st.captures == 1
    assert _bits(np.asarray(out), states[-1][0]) and _bits(np.asarray(mph.liquid_fraction), states[-1][1])
    log = mon.region_log()
    assert log['sum_extra'].shape == (2, 5)
    for s, (Ts, fs) in enumerate(states):
        want = hip.FieldMonitor.record_reference(Ts, mask, probes, regions, weights=mon.weights, ids=ids, extra=fs)
        assert _bits(log['sum_extra'][:, s], want['sum_extra']), s
        assert _bits(log['sum_T'][:, s], want['sum_T']) and _bits(log['heat'][:, s], want['sum_wT']), s
    assert (log['sum_extra'] > 0).all() and not _bits(log['sum_extra'][:, 0], log['sum_extra'][:, 4])
    assert np.isfinite(np.asarray(hist.T_peak)[mask]).all()


@pytest.mark.parametrize('cfl,theta', [(0.3, 0.5), (0.3, 1.0), (200.0, 1.0)])
def test_enthalpy_over_twenty_replayed_steps(hip, cfl, theta):
    """an adiabatic three-material body, latent heat on: over 20 steps replayed from the graph the enthalpy sum rho_m (cp_m T +
    L_m f) moves by at most 20 (N + 8) eps64 sum rho_m (cp_m |T| + L_m) -- the bar of the CPU test per step, the scale taken from
    the initial field.  cfl 200 runs at theta = 1: at theta = 0.5 the several-materials step itself, by its NumPy definition and
    with or without the correction, multiplies max|T| of this rough field (random holes, random ids, white noise) by 27 per step at
    cfl 200 (3e4 after one step, 1e30 after twenty), so no bar in units of the initial enthalpy can hold over 20 steps there; one
    step at theta = 0.5 and cfl 200 is held to the bar in tests/test_matmap_extras_cpu.py."""
    c = mc.case(HOLES_KEY)
    mask, ids, mats = c['mask'], np.array(c['ids']), c['materials']
    grid = hip.Grid3D(*c['shape'], mc.DX, mask)
    mm = hip.MaterialMap(grid, mats, ids)
    rng = np.random.default_rng(41)
    T0 = rng.uniform(900.0, 1700.0, c['shape'])
    mph = hip.MapPhaseField(mm, xc.LAWS, T=hip.to_device(T0))
    f0 = np.asarray(mph.liquid_fraction)
    prm = hip.Params(cfl * mc.DX ** 2 / mc.ALPHA_MAX, theta)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, mc.TINF, material_map=mm, phase=mph)
    T = np.asarray(st.run(hip.to_device(T0), 20))
    f = np.asarray(mph.liquid_fraction)
    assert st.captures == 1 and not _bits(f, f0)
    h0, scale = xc.enthalpy(T0, f0, mask, ids, mats)
    h1, _ = xc.enthalpy(T, f, mask, ids, mats)
    bar = 20 * (int(mask.sum()) + 8) * mc.EPS64 * scale
    print('cfl %g theta %g: enthalpy moves by %.3e over 20 steps, bar %.3e' % (cfl, theta, float(abs(h1 - h0)), float(bar)))
    assert abs(h1 - h0) <= bar


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_are_raised_before_any_launch(hip):
    c, grid, mm, prm, laws, losses, fl, T0, lp = _step_case(hip, HOLES_KEY)
    mask, ids, mats = c['mask'], np.array(c['ids']), c['materials']
    T = hip.to_device(T0)
    before = T.get()
    mph = hip.MapPhaseField(mm, laws, T=T)
    f_before = np.asarray(mph.liquid_fraction)
    coeff_before = [np.array(mm.packs[a].coeff) for a in range(3)]
    step = lambda *a, **kw: hip.adi_step_numba_coeff(T, *a, **kw)
    steel = hip.Material(*mc.STEEL)
    # the one-material objects with a map: "one cp"
    plain_lp = hip.LossPacks(grid, steel, xc.LOSSES[0], c['Tinf'])
    plain_ph = hip.PhaseField(grid, steel, xc.LAWS[0], T=T)
    for kw in (dict(surface_loss=plain_lp), dict(phase=plain_ph), dict(surface_loss=lp, phase=plain_ph),
               dict(surface_loss=plain_lp, phase=mph), dict(material=object())):
        with pytest.raises(ValueError, match='one cp'):
            step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, **kw)
        with pytest.raises(ValueError, match='one cp'):
            hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, **kw)
    # the new types without a map
    packs = hip.precompute_coeff_packs_unified(grid, steel, robin_h=350.0)
    with pytest.raises(TypeError, match='LossPacks'):
        step(grid, steel, prm, packs, c['Tinf'], surface_loss=lp)
    with pytest.raises(TypeError, match='PhaseField'):
        step(grid, steel, prm, packs, c['Tinf'], phase=mph)
    with pytest.raises(TypeError, match='PhaseField'):
        hip.StagedStepper(grid, steel, prm, packs, c['Tinf'], phase=mph)
    # another map's objects
    mm2 = hip.MaterialMap(grid, mats, ids, **dict(mc.bc_of(c), robin_h=None))
    with pytest.raises(ValueError, match='another MaterialMap'):
        step(grid, mm2.mat, prm, mm2.packs, c['Tinf'], material_map=mm2, surface_loss=lp)
    with pytest.raises(ValueError, match='another MaterialMap'):
        step(grid, mm2.mat, prm, mm2.packs, c['Tinf'], material_map=mm2, phase=mph)
    # a map built with robin_h
    mm3 = hip.MaterialMap(grid, mats, ids, robin_h=350.0)
    with pytest.raises(ValueError, match='robin_h'):
        hip.MapLossPacks(mm3, losses, c['Tinf'])
    # laws and losses of the wrong length or kind; an ambient at or below 0 K
    with pytest.raises(ValueError, match='2 laws for 3 materials'):
        hip.MapPhaseField(mm, laws[:2])
    with pytest.raises(TypeError, match='PhaseChange or None'):
        hip.MapPhaseField(mm, (laws[0], 1400.0, None))
    with pytest.raises(ValueError, match='2 losses for 3 materials'):
        hip.MapLossPacks(mm, losses[:2], c['Tinf'])
    with pytest.raises(TypeError, match='SurfaceLoss'):
        hip.MapLossPacks(mm, (losses[0], None, losses[2]), c['Tinf'])
    with pytest.raises(ValueError, match='kelvin'):
        hip.MapLossPacks(mm, losses, -300.0)
    with pytest.raises(ValueError, match='kelvin'):
        lp.update(T, Tinf=-300.0)
    with pytest.raises(TypeError, match='MaterialMap'):
        hip.MapPhaseField(grid, laws)
    # nothing above launched anything on the step's state
    assert _bits(T.get(), before) and _bits(np.asarray(mph.liquid_fraction), f_before)
    assert all(_bits(mm.packs[a].coeff, coeff_before[a]) for a in range(3))
    # a stale MapPhaseField: after set_ids, and after grid.mask changed (the map itself rebuilt)
    mm.set_ids(np.roll(ids, 3, axis=0))
    with pytest.raises(ValueError, match='sync_mask'):
        step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, phase=mph)
    mph.sync_mask(T)
    mask2 = np.array(mask); mask2[:, :, 33:] = False
    grid.mask = mask2
    mm.rebuild()
    with pytest.raises(ValueError, match='sync_mask'):
        step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, phase=mph)
    assert _bits(T.get(), before)
    mph.sync_mask(T)
    step(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, surface_loss=lp, phase=mph)
