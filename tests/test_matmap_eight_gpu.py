"""GPU: the step on a grid of several materials with all eight materials (ids 0 .. 7) at every device site that is built around the
8-wide tables -- the sweeps' pair table and its packed byte per row, the C table of the coefficient builds and of the source, the
law tables of the latent heat and the surface loss, the monitor's weights, the deposit's stamp -- and the segment kernels on either
side of every row count at which their build changes, on the layout the case names.  Cases, metric and bar:
tests/matmap_eight_cases.py; the conditions those cases rest on: tests/test_matmap_eight_cpu.py.  Every figure is printed before it
is asserted."""
import ctypes

import numpy as np
import pytest

import bead_cases as bc
import matmap_deposit_cases as dc
import matmap_eight_cases as ec
import matmap_extras_cases as xc
import matmap_ref_ld
from adi_thermal_fields_amd.packs import _nbr_in_mask

pytestmark = pytest.mark.gpu

LD = np.longdouble
KEY = ('eight', ec.HOLES, 'padded', None, 0.5, 200.0)               # the (20, 18, 35) case of the pointwise tests
KEY_CFL03 = ('eight', ec.HOLES, 'padded', None, 0.5, 0.3)
KEY_THETA1 = ('eight', ec.HOLES, 'padded', None, 1.0, 200.0)
assert {KEY, KEY_CFL03, KEY_THETA1} <= set(ec.eight_keys())


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def _layout(hip, monkeypatch, layout):
    if layout == 'padded':
        monkeypatch.setattr(hip, 'recommended_dims', ec.pad_dims)
    elif layout == 'exact':
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx, ny, nz))


def _setup(hip, c, **bc_kw):
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    mm = hip.MaterialMap(grid, c['materials'], np.array(c['ids']), **dict(ec.bc_of(c), **bc_kw))
    return grid, mm, hip.Params(c['dt'], c['theta'])


def _step(hip, c, grid, mm, prm, **kw):
    return np.asarray(hip.adi_step_numba_coeff(np.array(c['T0']), grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, **kw))


def _hold(X, c, ref, what):
    X = np.asarray(X)
    assert np.all(np.isfinite(X)), what
    ok, f = ec.meets_bar(X, c, ref)
    b = ec.bar(f, ec.A_MAP)
    print('%-72s inc %.2e K  err %.2e K = %8.2f ulp = %.1e inc = %.2e of the bar %.2e' % (what, f['inc'], f['abs_err'], f['ulp'],
                                                                                       f['of_inc'], f['abs_err'] / b, b))
    assert ec.untouched_exact(X, c), what
    assert ok, (what, f)


def _hold_stage(got, want, X0, c, what):
    """the bar of one step applied to one sweep: its own input X0 in place of T0"""
    mask = c['mask']
    dirc = mask & c['dir_mask']
    free = mask & ~dirc
    err = float(np.max(np.abs(got - want)[mask]))
    inc = float(np.max(np.abs(want - X0)[free]))
    wmax = float(np.max(np.abs(want[mask])))
    b = ec.A_MAP * ec.EPS64 * wmax + 1e-10 * inc
    print('%-72s inc %.2e K  err %.2e K = %8.2f ulp = %.2e of the bar %.2e' % (what, inc, err, err / (ec.EPS64 * wmax), err / b, b))
    assert np.all(np.isfinite(got)), what
    assert np.array_equal(got[~mask], X0[~mask]), what
    assert np.array_equal(got[dirc], c['dir_value'][dirc]), what
    assert err <= b, (what, err, b)


def _definition(c, **kw):
    from adi_thermal_fields_amd.packs import MaterialMap
    return ec.run(MaterialMap.step_reference, MaterialMap.packs_reference, c, **kw)


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _raw(t):
    n = t.untyped_storage().nbytes() // t.element_size()
    return t.as_strided((n,), (1,))


def _six(mm):
    return [p.d_coeff for p in mm.packs] + [p.d_qflux for p in mm.packs]


# ---- 1. one step against the long-double reference ------------------------------------------------------------------------------
@pytest.mark.parametrize(**ec.params(ec.eight_keys()))
def test_one_step_eight_materials(hip, monkeypatch, key):
    _layout(hip, monkeypatch, key[2])
    c = ec.case(key)
    grid, mm, prm = _setup(hip, c)
    if key[2] == 'padded':
        assert grid.layout.padded and grid.layout.pd[:3] == ec.pad_dims(*c['shape'])
    _hold(_step(hip, c, grid, mm, prm), c, ec.reference(key), ec.tag(key))


@pytest.mark.parametrize(**ec.params(ec.switch_keys()))
def test_one_step_and_the_sweep_under_test_at_every_switch(hip, monkeypatch, key):
    from adi_thermal_fields_amd import _lib
    _layout(hip, monkeypatch, key[2])
    axis = key[3]
    c = ec.case(key)
    n = c['shape'][axis]
    grid, mm, prm = _setup(hip, c)
    assert grid.layout.pd[:3] == c['shape'] and not grid.layout.padded      # the kernel sees the length the case names
    work = ctypes.c_size_t(7)
    _lib.check(_lib.lib.adi_matmap_workspace_bytes(axis, *grid.layout.pd, ctypes.byref(work)))
    if n == 1025:
        assert work.value > 0 and mm._work is not None and mm._work.numel() >= work.value
    if n <= 1024:
        assert work.value == 0
    _hold(_step(hip, c, grid, mm, prm), c, ec.reference(key), ec.tag(key))
    # the sweep of the axis alone, from the definition's fp64 input of that stage: a full step can smear a one-row error of the
    # first sweep over the line, this cannot
    _, st64 = _definition(c, return_stages=True)
    X = np.array(st64[('R0', 'U', 'V')[axis]])
    mask = c['mask']
    idm = np.where(mask, c['ids'], 0).astype(np.intp)
    pk = matmap_ref_ld.packs(mask, c['ids'], c['materials'], c['dx'], **ec.bc_of(c))
    G = matmap_ref_ld.pair_table(c['materials'], c['dx'], c['dt'])
    got = np.asarray(mm.sweep_axis(axis, X, prm, c['Tinf']))
    want = matmap_ref_ld.sweep(axis, X.astype(LD), mask, idm, LD(c['theta']) * G, c['dt'], pk[axis], c['Tinf'])
    _hold_stage(got, want, X, c, 'sweep ' + ec.tag(key))


# ---- 2. packs -------------------------------------------------------------------------------------------------------------------
def test_packs_rebuild_and_update_bit_equal_to_the_definition_and_nothing_outside_the_range(hip, monkeypatch):
    import torch
    _layout(hip, monkeypatch, 'padded')
    c = ec.case(KEY)
    mask = np.array(c['mask'])
    grid, mm, prm = _setup(hip, c)
    L = grid.layout
    assert L.padded and L.pz > L.nz

    def same_as_the_definition(mm, mask, what):
        want = hip.MaterialMap.packs_reference(mask, c['ids'], c['materials'], c['dx'], **ec.bc_of(c))
        for a in range(3):
            assert _bits(mm.packs[a].coeff, want[a].coeff), (what, a)
            assert _bits(mm.packs[a].qflux, want[a].qflux), (what, a)
            assert want[a].coeff.any() and want[a].qflux.any() == (a != 0)
        return want

    w1 = same_as_the_definition(mm, mask, 'rebuild')
    C = np.array([rho * cp for rho, cp, _ in c['materials']])[c['ids']]
    for m in range(8):                                       # every material owns cells whose coefficient is not zero
        assert all((w1[a].coeff[mask & (c['ids'] == m)] != 0).any() for a in range(3)), m
    assert len(set(C.ravel().tolist())) == 8
    # a mask change on the planes [11, 15): cells join and leave; the planes either side see new neighbours
    rng = np.random.default_rng(19)
    mask2 = mask.copy()
    mask2[:, :, 11:15] ^= rng.random(mask[:, :, 11:15].shape) < 0.3
    k0, k1 = 10, 16
    grid.mask = mask2
    assert mm.update(k0, k1) is mm.packs
    w2 = same_as_the_definition(mm, mask2, 'update')
    assert not _bits(w2[2].coeff, w1[2].coeff) and _bits(w2[2].coeff[:, :, :k0], w1[2].coeff[:, :, :k0])
    # ... and not a byte outside the range
    good = [_raw(x).clone() for x in _six(mm)]
    inside = torch.zeros(L.numel_padded, dtype=torch.bool, device='cuda')
    inside.as_strided((L.px, L.py, L.pz), (L.sx, L.pz, 1))[:, :, k0:k1] = True
    for x in _six(mm):
        _raw(x).fill_(float('nan'))
    sentinel = _raw(_six(mm)[0]).clone().view(torch.int64)
    mm.update(k0, k1)
    for x, ok in zip(_six(mm), good):
        now = _raw(x).view(torch.int64)
        assert torch.equal(now[~inside], sentinel[~inside])
        assert torch.equal(now[inside], ok.view(torch.int64)[inside])
    assert inside.any() and (~inside).any()
    mm.rebuild()
    same_as_the_definition(mm, mask2, 'rebuild after the update')


# ---- 3. source ------------------------------------------------------------------------------------------------------------------
def test_source_field_and_map_source_on_eight_materials(hip, monkeypatch):
    _layout(hip, monkeypatch, 'padded')
    c = ec.case(KEY_CFL03)
    grid, mm, prm = _setup(hip, c)
    assert grid.layout.padded
    # the field form against the reference
    S = ec.source_field(KEY_CFL03)
    ref = ec.reference_of(c, S=S)
    _hold(_step(hip, c, grid, mm, prm, S=S), c, ref, 'S as a field, eight materials')
    assert not np.array_equal(ref[0], ec.reference(KEY_CFL03)[0])
    # MapSource against the field form, bit for bit
    t = 0.013
    src = hip.GoldakSource(origin=(9.9e-3 - 0.01 * t, 9.2e-3, 35e-3), **dc.SRC_KW)
    msrc = hip.MapSource(mm, src)
    tm = t + 0.5 * prm.dt
    q = src.sample(grid, tm)
    counts = [int(((q > 0) & c['mask'] & (c['ids'] == m)).sum()) for m in range(8)]
    print('in-mask cells of each material in the support: %s' % counts)
    assert min(counts) >= 20
    d_S = src.sample_device(grid, tm)
    T0 = np.array(c['T0'])
    got = np.asarray(msrc.explicit_rhs(T0, prm, t=t))
    field = np.asarray(mm.explicit_rhs(T0, prm, S=d_S))
    plain = np.asarray(mm.explicit_rhs(T0, prm))
    print('R0: source form bit-equal to the field form: %s' % _bits(got, field))
    assert _bits(got, field) and not _bits(got, plain)
    X = _step(hip, c, grid, mm, prm, S=msrc, t=t)
    F = _step(hip, c, grid, mm, prm, S=d_S)
    print('step: source form bit-equal to the field form: %s' % _bits(X, F))
    assert _bits(X, F)
    _hold(X, c, ec.reference_of(c, S=dc.source_field_ld(src, c['shape'], c['dx'], c['mask'], tm)), 'step with MapSource, eight materials')


# ---- 4. phase -------------------------------------------------------------------------------------------------------------------
def test_seed_and_apply_on_bricks8_bit_equal_to_the_definition(hip):
    import torch
    mask, ids = (np.array(a) for a in ec.bricks8())
    mats = ec.MATERIALS8
    laws = xc.laws_of(mats)
    grid = hip.Grid3D(*ec.BRICKS_SHAPE, ec.DX, mask)
    mm = hip.MaterialMap(grid, mats, ids)
    fl = xc.fields(mask, ids, laws)
    xc.assert_covered(fl['T_star'], fl['f0'], mask, ids, fl['dir_mask'], mats, 'bricks8')      # (on the CPU, before any launch)
    pd = grid.layout.pd[:3]
    assert pd == ec.BRICKS_SHAPE
    want_ids = xc.brick_words(mask, ids, pd)
    assert want_ids[:8].tolist() == [1 << b for b in range(8)] and want_ids[11] == 0 and (want_ids[12:] == 255).all()
    # T that no kernel may read: the brick without an in-mask cell and the bricks of the two materials without a law
    T_seed, T_star = np.array(fl['T_seed']), np.array(fl['T_star'])
    for b in [11] + [m for m in range(8) if laws[m] is None]:
        sl = (slice(16 * (b // 8), 16 * (b // 8) + 16), slice(16 * ((b // 4) % 2), 16 * ((b // 4) % 2) + 16),
              slice(16 * (b % 4), 16 * (b % 4) + 16))
        T_seed[sl] = np.nan
        T_star[sl] = np.nan
    words = lambda t: t.cpu().numpy()                                  # noqa: E731
    # seed
    mph = hip.MapPhaseField(mm, laws, T=hip.to_device(T_seed))
    f0 = xc.MapPhaseField.f_eq_of(laws, T_seed, mask, ids)
    assert _bits(f0, fl['f0'])
    assert _bits(np.asarray(mph.liquid_fraction), f0)
    assert np.array_equal(words(mph.summary), xc.brick_any(f0, pd))
    assert np.array_equal(words(mph.brick_ids), want_ids)
    # apply, with Dirichlet cells
    T = hip.to_device(T_star)
    mph.apply(T, grid.layout.to_layout(fl['dir_mask'], torch.uint8))
    want_T, want_f = xc.MapPhaseField.correct_of(laws, mats, T_star, f0, mask, ids, fl['dir_mask'])
    got_T, got_f = np.asarray(T), np.asarray(mph.liquid_fraction)
    for m in range(8):
        cells = mask & (ids == m)
        bad = int((got_T.view(np.uint64) != want_T.view(np.uint64))[cells].sum()), int((got_f != want_f)[cells].sum())
        changed = int((want_T.view(np.uint64) != T_star.view(np.uint64))[cells].sum())
        print('material %d: %d cells, the definition changes T in %d; T differs in %d, f in %d' % (m, cells.sum(), changed, *bad))
        assert (changed > 0) == (laws[m] is not None)
    assert _bits(got_T, want_T) and _bits(got_f, want_f)
    assert np.array_equal(words(mph.summary), xc.brick_any(want_f, pd))
    assert np.array_equal(words(mph.brick_ids), want_ids)
    # a second pass from the state the first left, without Dirichlet cells
    mph.apply(T)
    want_T2, want_f2 = xc.MapPhaseField.correct_of(laws, mats, want_T, want_f, mask, ids, None)
    assert _bits(np.asarray(T), want_T2) and _bits(np.asarray(mph.liquid_fraction), want_f2)
    assert np.array_equal(words(mph.summary), xc.brick_any(want_f2, pd))
    assert not _bits(want_T2, want_T)


# ---- 5. loss --------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def test_loss_update_and_rebuild_with_eight_laws_bit_equal_to_the_definition(hip):
    c = ec.case(KEY)
    mask, ids, mats = c['mask'], np.array(c['ids']), c['materials']
    losses = xc.losses_of(mats)
    grid, mm, prm = _setup(hip, c, robin_h=None)
    T = np.random.default_rng(31).uniform(100.0, 1900.0, c['shape'])   # below the first knot of every table and beyond its last
    Td = hip.to_device(T)
    lp = hip.MapLossPacks(mm, losses, xc.TINF)
    for a in range(3):
        mm.packs[a].d_coeff.fill_(SENTINEL)
    lp.update(Td)
    want = hip.MapLossPacks.coeff_reference(T, mask, ids, mats, ec.DX, losses, xc.TINF)
    for a in range(3):
        ex = mask & ~(_nbr_in_mask(mask, a, False) & _nbr_in_mask(mask, a, True))
        got = mm.packs[a].coeff
        for m in range(8):
            cells = ex & (ids == m)
            n = int((got[cells].view(np.uint64) != want[a][cells].view(np.uint64)).sum())
            print('axis %d material %d: %d exposed cells, %d differ' % (a, m, cells.sum(), n))
            assert cells.sum() >= 100
        assert _bits(got[ex], want[a][ex]), a
        assert (got[~ex] == SENTINEL).all(), a
        assert (want[a][ex] > 0).any() and (want[a][ex] == 0).any()   # some laws lose nothing on some face
    lp.rebuild(Td)
    for a in range(3):
        assert _bits(mm.packs[a].coeff, want[a]), a
    # every material's own law: the field differs from the one that any other single law would give
    for m in range(8):
        only = hip.MapLossPacks.coeff_reference(T, mask, ids, mats, ec.DX, losses[m], xc.TINF)
        assert any(not _bits(only[a][mask & (ids != m)], want[a][mask & (ids != m)]) for a in range(3)), m


# ---- 6. monitor -----------------------------------------------------------------------------------------------------------------
def test_monitor_heat_content_under_an_eight_material_map(hip):
    shape = (32, 32, 48)
    rng = np.random.default_rng(61)
    mask = rng.random(shape) > 0.25
    ids = ec.random8(rng, shape)
    T0 = rng.uniform(20.0, 1500.0, shape)
    grid = hip.Grid3D(*shape, ec.DX, mask)
    mm = hip.MaterialMap(grid, ec.MATERIALS8, ids, robin_h=350.0)
    FM = hip.FieldMonitor
    regions = (None, ((3, 29), (5, 30), (7, 41)))                      # the whole grid, and a box that cuts bricks on every side
    probes = ((0, 0, 0), (17, 9, 40), (31, 31, 47))
    mon = FM(grid, probes=probes, regions=regions, capacity=4, material_map=mm)
    w = FM.weights_of(mm.materials, ec.DX)
    assert mon.weights == w and len(set(w)) == 8
    prm = hip.Params(0.3 * ec.DX ** 2 / ec.ALPHA_MAX, 0.5)
    T = hip.to_device(T0)
    mon.record(T, 0.0)
    fields = [T0]
    for _ in range(2):
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, ec.TINF, material_map=mm, monitor=mon)
        fields.append(np.asarray(T))
    rows, dropped = mon.rows()
    assert dropped == 0 and len(rows) == 3
    for s, (row, F) in enumerate(zip(rows, fields)):
        ref = FM.record_reference(F, mask, probes, regions, weights=w, ids=ids)
        want = FM.row_of(ref)
        bad = np.flatnonzero(row != want)
        print('row %d: heat %s J, %d words differ' % (s, ref['sum_wT'].tolist(), bad.size))
        assert bad.size == 0, (s, bad.tolist(), row[bad].view(np.float64).tolist(), want[bad].view(np.float64).tolist())
        # ids cut to two bits, or every cell weighted as material 0, would log another heat content
        for wrong in (FM.record_reference(F, mask, probes, regions, weights=w, ids=ids & 3),
                      FM.record_reference(F, mask, probes, regions, weights=w, ids=np.zeros_like(ids))):
            assert not _bits(wrong['sum_wT'], ref['sum_wT'])
    log = mon.region_log()
    assert _bits(log['heat'][:, 2], FM.record_reference(fields[2], mask, probes, regions, weights=w, ids=ids)['sum_wT'])


# ---- 7. deposit -----------------------------------------------------------------------------------------------------------------
def test_deposits_of_wires_7_and_4_on_an_eight_material_map(hip):
    import torch
    a, b = bc.BY_NAME['leg_plus_u'], bc.BY_NAME['leg_plus_v']
    assert a.shape == b.shape
    ids0 = dc.random_ids(a.shape, 3, n=8)
    assert set(np.unique(ids0).tolist()) == set(range(8))
    kw = dict(robin_h=dc.voxel_h(a.shape), neumann=dc.FLUX)
    g = hip.Grid3D(*a.shape, bc.DX, a.active)
    mm = hip.MaterialMap(g, ec.MATERIALS8, ids0, **kw)
    T = hip.to_device(np.full(a.shape, 300.0))
    mask, ids = a.active.copy(), ids0
    for case, wire in ((a, 7), (b, 4)):
        dep = hip.PathDeposit(g, case.path, case.bead, bc.TS, material_map=mm, material_id=wire)
        born = case.reference(*case.whole(), active=mask)
        rng = dep.deposit(T, *case.whole())
        assert born.any() and rng is not None
        mask, ids = mask | born, dc.stamp(ids, born, wire)
        np.testing.assert_array_equal(g.d_mask.cpu().numpy().astype(bool), mask)
        np.testing.assert_array_equal(mm.ids, ids)
        np.testing.assert_array_equal(mm._d_ids.cpu().numpy(), ids)
        if wire == 7:
            want_mask, want_ids = dc.births_and_ids(a, [a.whole()], ids0, material_id=7)
            np.testing.assert_array_equal(want_mask, mask)
            np.testing.assert_array_equal(want_ids, ids)
        assert mm.update(*rng) is mm.packs
        fresh = hip.MaterialMap(hip.Grid3D(*a.shape, bc.DX, mask), ec.MATERIALS8, ids, **kw)
        want = hip.MaterialMap.packs_reference(mask, ids, ec.MATERIALS8, bc.DX, **kw)
        for ax in range(3):
            assert _bits(mm.packs[ax].coeff, want[ax].coeff) and _bits(mm.packs[ax].qflux, want[ax].qflux), (wire, ax)
        for x, y in zip(_six(mm), _six(fresh)):                # the physical box, plane padding included
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), wire
    assert int((ids == 7).sum()) > int((ids0 == 7).sum()) and int((ids == 4).sum()) > int((ids0 == 4).sum())
    # a step on the grid as the deposits left it, against the definition
    prm = hip.Params(1e-3, 0.5)
    got = np.asarray(hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, 300.0, material_map=mm))
    c = dict(shape=a.shape, dx=bc.DX, materials=ec.MATERIALS8, mask=mask, ids=ids, T0=np.asarray(T), dir_mask=None, dir_value=None,
             Tinf=300.0, theta=0.5, dt=prm.dt, **kw)
    _hold(got, dict(c, dir_mask=np.zeros(a.shape, bool)), ec.reference_of(c), 'a step after the two deposits')


# ---- 8. graph -------------------------------------------------------------------------------------------------------------------
def test_graph_replay_of_six_steps_is_six_plain_steps(hip, monkeypatch):
    _layout(hip, monkeypatch, 'padded')
    c = ec.case(KEY_THETA1)
    grid, mm, prm = _setup(hip, c)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
    T = hip.to_device(c['T0'])
    for _ in range(6):
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm)
    six = T.get()
    got = st.run(hip.to_device(c['T0']), 6).get()
    assert st.captures == 1 and _bits(got, six)
    assert np.all(np.isfinite(six)) and not _bits(six, np.array(c['T0']))
    _hold(st.step(hip.to_device(c['T0'])).get(), c, ec.reference(KEY_THETA1), 'StagedStepper.step, eight materials')
