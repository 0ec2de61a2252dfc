"""GPU: a MaterialMap carried through deposits and a moving source: MaterialMap.update on the plane range of a
deposit against a fresh build and the NumPy definition; the id stamp of PathDeposit(material_map=, material_id=) against
where(reference, id, ids); MapSource inside the step against the field form, the long-double reference and its energy; the
graph replay; and the three waam drivers with material_map= against the same sequence by hand and the NumPy definition loop
(matmap_deposit_cases.definition_loop).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import bead_cases as bc
import matmap_cases as mc
import matmap_deposit_cases as dc
from bead_cases import CASES, DX, TS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _raw(t):
    n = t.untyped_storage().nbytes() // t.element_size()
    return t.as_strided((n,), (1,))


def _mask_of(g):
    return g.d_mask.cpu().numpy().astype(bool)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _bc(shape, form):
    return dict(robin_h=dc.ROBIN if form == 'dict' else dc.voxel_h(shape), neumann=dc.FLUX)


def _six(mm):
    return [p.d_coeff for p in mm.packs] + [p.d_qflux for p in mm.packs]


def _map_on(hip, case, form, ids=None):
    g = hip.Grid3D(*case.shape, DX, case.active)
    ids = dc.random_ids(case.shape, 3) if ids is None else ids
    return g, hip.MaterialMap(g, dc.MATERIALS, ids, **_bc(case.shape, form)), ids


# ---------------------------------------------------------------------------------------------------------- 1. plane update
@pytest.mark.parametrize('form', ['dict', 'voxel'])
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_update_after_every_deposit_equals_a_fresh_build_and_the_definition(hip, case, form):
    import torch
    g, mm, ids = _map_on(hip, case, form)
    T = hip.to_device(np.full(case.shape, 300.0))
    dep = hip.PathDeposit(g, case.path, case.bead, TS, within=case.within, material_map=mm, material_id=dc.WIRE)
    mask = case.active.copy()
    for t, dt in list(case.windows) + [case.whole()]:
        born = case.reference(t, dt, active=mask)
        rng = dep.deposit(T, t, dt)
        mask, ids = mask | born, dc.stamp(ids, born, dc.WIRE)
        if rng is None:
            assert not born.any()
            continue
        assert mm.update(*rng) is mm.packs
        assert all(p.mask_version == g.mask_version for p in mm.packs)
        fresh_g = hip.Grid3D(*case.shape, DX, mask)
        fresh = hip.MaterialMap(fresh_g, dc.MATERIALS, ids, **_bc(case.shape, form))
        want = hip.MaterialMap.packs_reference(mask, ids, dc.MATERIALS, DX, **_bc(case.shape, form))
        for a in range(3):
            assert np.array_equal(mm.packs[a].coeff, want[a].coeff) and np.array_equal(mm.packs[a].qflux, want[a].qflux), a
        for x, y in zip(_six(mm), _six(fresh)):              # the physical box, plane padding included
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    np.testing.assert_array_equal(mm.ids, ids)


RANGES = {'first_plane': lambda nz, pz: (0, 1), 'ends_at_nz': lambda nz, pz: (nz - 3, nz),
          'into_the_padding': lambda nz, pz: (nz - 2, pz + 5)}


@pytest.mark.parametrize('which', sorted(RANGES))
@pytest.mark.parametrize('name', ['corner', 'padded_by_the_library'])
def test_update_writes_its_range_and_not_a_byte_outside(hip, monkeypatch, name, which):
    import torch
    case = bc.BY_NAME[name]
    if name == 'corner':
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx + 4, ny + 4, nz + 4))
    g, mm, ids = _map_on(hip, case, 'voxel')
    L = g.layout
    assert L.padded and L.pz > L.nz
    good = [_raw(x).clone() for x in _six(mm)]
    k0, k1 = RANGES[which](L.nz, L.pz)
    inside = torch.zeros(L.numel_padded, dtype=torch.bool, device='cuda')
    inside.as_strided((L.px, L.py, L.pz), (L.sx, L.pz, 1))[:, :, max(0, k0):min(L.pz, k1)] = True
    nan = float('nan')
    for x in _six(mm):
        _raw(x).fill_(nan)
    sentinel = _raw(_six(mm)[0]).clone().view(torch.int64)
    mm.update(k0, k1)
    for x, ok in zip(_six(mm), good):
        now = _raw(x)
        assert torch.equal(now.view(torch.int64)[~inside], sentinel[~inside])       # outside: the sentinel's bytes
        assert torch.equal(now.view(torch.int64)[inside], ok.view(torch.int64)[inside])   # inside: the full build's, zeros included
    assert inside.any() and (~inside).any()


def test_a_deposit_that_bears_nothing_launches_nothing(hip):
    import torch
    case = bc.BY_NAME['wholly_outside']
    g, mm, ids = _map_on(hip, case, 'dict')
    T = hip.to_device(np.full(case.shape, 300.0))
    dep = hip.PathDeposit(g, case.path, case.bead, TS, material_map=mm, material_id=2)
    version, before = g.mask_version, [x.clone() for x in _six(mm)]
    assert dep.deposit(T, *case.whole()) is None
    assert g.mask_version == version and all(torch.equal(x, y) for x, y in zip(_six(mm), before))
    np.testing.assert_array_equal(mm.ids, ids)


def test_update_refuses_an_invalid_id_off_the_mask_and_rebuild_serves_it(hip):
    case = bc.BY_NAME['corner']
    ids = dc.random_ids(case.shape, 3)
    ids[~case.active] = 255
    g = hip.Grid3D(*case.shape, DX, case.active)
    mm = hip.MaterialMap(g, dc.MATERIALS, ids, robin_h=dc.ROBIN)
    assert not mm.ids_all_valid
    with pytest.raises(ValueError, match='update'):
        mm.update(0, 3)
    mm.rebuild()
    mm.set_ids(dc.random_ids(case.shape, 3))
    assert mm.ids_all_valid and mm.update(0, 3) is mm.packs


def test_a_step_right_after_update_runs(hip):
    case = bc.BY_NAME['corner']
    g, mm, ids = _map_on(hip, case, 'dict')
    T = hip.to_device(np.full(case.shape, 300.0))
    dep = hip.PathDeposit(g, case.path, case.bead, TS, material_map=mm, material_id=dc.WIRE)
    prm = hip.Params(1e-3, 0.5)
    rng = dep.deposit(T, *case.whole())
    with pytest.raises(ValueError, match='call rebuild'):
        hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, 300.0, material_map=mm)
    mm.update(*rng)
    got = np.asarray(hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, 300.0, material_map=mm))
    mask = _mask_of(g)
    pk = hip.MaterialMap.packs_reference(mask, mm.ids, dc.MATERIALS, DX, robin_h=dc.ROBIN, neumann=dc.FLUX)
    want = hip.MaterialMap.step_reference(np.asarray(T), mask, mm.ids, dc.MATERIALS, DX, prm.dt, 0.5, pk, 300.0)
    err = rel_linf(got, want)
    print('step after update vs the definition: %.2e' % err)
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ 2. stamp
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_stamp_equals_the_definition(hip, case):
    import torch
    ids = dc.random_ids(case.shape, 7)
    g = hip.Grid3D(*case.shape, DX, case.active)
    mm = hip.MaterialMap(g, dc.MATERIALS, ids, robin_h=dc.ROBIN)
    rng0 = np.random.default_rng(7)
    T0 = rng0.uniform(300.0, 900.0, case.shape)
    T = hip.to_device(T0)
    dep = hip.PathDeposit(g, case.path, case.bead, TS, within=case.within, material_map=mm, material_id=2)
    count = torch.full((1,), -7, dtype=torch.int64, device='cuda')
    mask = case.active.copy()
    key = mm.graph_key()
    for t, dt in case.windows:
        want = case.reference(t, dt, active=mask)
        pad_before = _raw(mm._d_ids).clone()
        rng = dep.deposit(T, t, dt, count=count)
        ids = dc.stamp(ids, want, 2)
        np.testing.assert_array_equal(_mask_of(g), mask | want)
        assert int(count.item()) == int(want.sum())
        now = np.asarray(T)
        assert (now[want] == TS).all()
        np.testing.assert_array_equal(_bits(now[~want]), _bits(T0[~want]))
        np.testing.assert_array_equal(mm.ids, ids)                                # downloads the stamped field
        np.testing.assert_array_equal(mm._d_ids.cpu().numpy(), ids)
        prev = _prev_ids(pad_before, g)
        changed = _raw(mm._d_ids) != pad_before                                   # the whole storage, padding included
        assert int(changed.sum().item()) == int((want & (prev != 2)).sum())       # no byte but a newborn cell's changed
        assert (rng is None) == (dep.index_box(t, dt) is None)
        mask |= want
        T0 = np.where(want, TS, T0)
    assert mm.graph_key() == key                                                  # a stamp recaptures nothing


def _prev_ids(raw, g):
    L = g.layout
    return raw.as_strided(L.shape, L.strides).cpu().numpy()


def test_depositing_onto_active_cells_changes_no_id_and_a_second_wire_stamps_its_own(hip):
    a, b = bc.BY_NAME['leg_plus_u'], bc.BY_NAME['leg_plus_v']
    ids0 = dc.random_ids(a.shape, 9, n=1)                                          # all 0
    g = hip.Grid3D(*a.shape, DX, a.active)
    mm = hip.MaterialMap(g, dc.MATERIALS, ids0, robin_h=dc.ROBIN)
    T = hip.to_device(np.full(a.shape, 300.0))
    one = hip.PathDeposit(g, a.path, a.bead, TS, material_map=mm, material_id=1)
    two = hip.PathDeposit(g, b.path, b.bead, TS, material_map=mm, material_id=2)
    one.deposit(T, *a.whole())
    born_a = _mask_of(g) & ~a.active
    ids1 = mm.ids
    assert born_a.any() and np.array_equal(ids1, np.where(born_a, 1, ids0))
    again = hip.PathDeposit(g, a.path, a.bead, TS, material_map=mm, material_id=2)  # the same bead again: every cell is active
    again.deposit(T, *a.whole())
    np.testing.assert_array_equal(mm.ids, ids1)
    before = _mask_of(g)
    two.deposit(T, *b.whole())
    born_b = _mask_of(g) & ~before
    assert born_b.any() and np.array_equal(born_b, b.reference(*b.whole(), active=before))
    np.testing.assert_array_equal(mm.ids, np.where(born_b, 2, ids1))
    mm.set_ids(ids0)                                                                # replaces both copies
    np.testing.assert_array_equal(mm.ids, ids0)
    np.testing.assert_array_equal(mm._d_ids.cpu().numpy(), ids0)


# ----------------------------------------------------------------------------------------------------------------- 3. source
SRC_KEY = ('holes', mc.HOLES, 'random3', 'general', 0.5, 0.3)


def _src_case(shape=mc.HOLES, key=SRC_KEY, axis=0):
    c = dict(mc.case(key))
    c['ids'] = dc.interface_ids(shape, axis=axis)
    return c


def _src(hip, origin, **kw):
    return hip.GoldakSource(origin=origin, **dict(dc.SRC_KW, **kw))


def _setup(hip, c):
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    mm = hip.MaterialMap(grid, c['materials'], np.array(c['ids']), **mc.bc_of(c))
    return grid, mm, hip.Params(c['dt'], c['theta'])


def _hold(X, c, ref, what):
    X = np.asarray(X)
    ok, f = mc.meets_bar(X, c, ref)
    print('%-70s inc %.2e K  err %.2e K = %8.2f ulp  bar %.2e' % (what, f['inc'], f['abs_err'], f['ulp'], mc.bar(f, mc.A_MAP)))
    assert mc.untouched_exact(X, c), what
    assert ok, (what, f)


T_SRC = 0.013
ORIGIN = (9.9e-3 - 0.01 * (T_SRC), 9.2e-3, 35e-3)          # at the step's mid-time the centre sits on the interface, on the top face


def test_source_r0_and_step_against_the_field_form_the_reference_and_the_energy(hip, monkeypatch):
    monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx + 1, ny + 2, nz + 3))
    c = _src_case()
    grid, mm, prm = _setup(hip, c)
    assert grid.layout.padded
    src = _src(hip, ORIGIN)
    msrc = hip.MapSource(mm, src)
    t = T_SRC
    tm = t + 0.5 * prm.dt
    q = src.sample(grid, tm)
    for m in (0, 2):                                       # at least 20 in-mask cells of STEEL and of INSULATOR in the support
        n = int(((q > 0) & c['mask'] & (c['ids'] == m)).sum())
        print('in-mask cells of material %d in the support: %d' % (m, n))
        assert n >= 20
    T0 = np.array(c['T0'])
    d_S = src.sample_device(grid, tm)
    # R0
    got = msrc.explicit_rhs(T0, prm, t=t)
    field = mm.explicit_rhs(T0, prm, S=d_S)
    plain = mm.explicit_rhs(T0, prm)
    e = rel_linf(got, field)
    print('R0: source form vs field form %.2e, bit-equal %s' % (e, np.array_equal(got, field)))
    assert e <= 1e-12
    assert np.array_equal(got[~c['mask']], T0[~c['mask']]) and np.array_equal(got[q == 0], plain[q == 0])
    assert np.array_equal(got, field)                      # the same operations in the same order
    # energy: sum C_id (R0 - R0_without) dx^3 = dt sum q dx^3
    C = np.array([rho * cp for rho, cp, _ in c['materials']])[np.where(c['mask'], c['ids'], 0)]
    e_field = float(np.sum((C * (got - plain))[c['mask']]) * c['dx'] ** 3)
    e_in = float(prm.dt * np.sum(q[c['mask']]) * c['dx'] ** 3)
    print('energy: field %.15e J, input %.15e J, rel %.2e' % (e_field, e_in, abs(e_field - e_in) / e_in))
    assert abs(e_field - e_in) <= 1e-11 * e_in
    # the full step
    X = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=msrc, t=t))
    F = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=d_S))
    e = rel_linf(X, F)
    print('step: source form vs field form %.2e, bit-equal %s' % (e, np.array_equal(X, F)))
    assert e <= 1e-12
    ref = mc.reference_of(c, S=dc.source_field_ld(src, c['shape'], c['dx'], c['mask'], tm))
    _hold(X, c, ref, 'step with MapSource vs the long-double reference')
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, source=msrc)
    assert np.array_equal(st.step(hip.to_device(T0), t=t).get(), X)
    # one C for every cell would miss the bar by orders of magnitude
    wrong = plain + (got - plain) * (C / C.max())
    assert rel_linf(wrong, field) > 1e-6


def test_source_refusals_come_before_any_launch(hip):
    c = _src_case()
    grid, mm, prm = _setup(hip, c)
    grid2, mm2, _ = _setup(hip, c)
    src = _src(hip, ORIGIN)
    T = hip.to_device(c['T0'])
    before = T.get()
    plain_packs = hip.precompute_coeff_packs_unified(grid, mm.mat, robin_h=350.0)
    with pytest.raises(ValueError, match='needs material_map'):
        hip.adi_step_numba_coeff(T, grid, mm.mat, prm, plain_packs, c['Tinf'], S=hip.MapSource(mm, src))
    with pytest.raises(ValueError, match='needs material_map'):
        hip.StagedStepper(grid, mm.mat, prm, plain_packs, c['Tinf'], source=hip.MapSource(mm, src))
    with pytest.raises(ValueError, match='another MaterialMap'):
        hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=hip.MapSource(mm2, src))
    with pytest.raises(ValueError, match='GoldakSource'):
        hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=src)
    assert np.array_equal(T.get(), before)


FACES6 = [(a, s) for a in range(3) for s in (-1, 1)]


@pytest.mark.parametrize('axis,side', FACES6, ids=['%s%s' % ('xyz'[a], '-+'[s > 0]) for a, s in FACES6])
def test_source_clipped_at_each_face(hip, axis, side):
    """the centre one source length (c_r = 6 dx) outside the face: part of the support reaches into the grid; and far outside:
    the step without a source, bit for bit"""
    c = _src_case()
    grid, mm, prm = _setup(hip, c)
    T0 = np.array(c['T0'])
    ext = [n * c['dx'] for n in c['shape']]
    plain = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm))
    for dist, reaches in ((6e-3, True), (40e-3, False)):
        org = [0.5 * e for e in ext]
        org[2] = ext[2]
        org[axis] = -dist if side < 0 else ext[axis] + dist
        src = _src(hip, tuple(org), velocity=0.0)
        q = src.sample(grid, 0.0)
        assert bool((q > 0).any()) == reaches
        X = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=hip.MapSource(mm, src)))
        if reaches:
            F = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm,
                                                    S=src.sample_device(grid, 0.5 * prm.dt)))
            e = rel_linf(X, F)
            print('axis %d side %+d: source vs field %.2e' % (axis, side, e))
            assert e <= 1e-12 and not np.array_equal(X, plain)
        else:
            assert np.array_equal(X, plain)


def test_source_larger_than_the_grid_and_power_zero(hip):
    shape = bc.SHAPES[1]                                   # 13 x 11 x 9
    rng = np.random.default_rng(3)
    mask = rng.random(shape) > 0.2
    ids = dc.random_ids(shape, 4)
    grid = hip.Grid3D(*shape, DX, mask)
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=dc.ROBIN)
    prm = hip.Params(2e-3, 0.5)
    T0 = rng.uniform(300.0, 900.0, shape)
    big = hip.GoldakSource(power=900.0, eta=0.8, a=9e-3, b=8e-3, c_f=9e-3, c_r=15e-3, origin=(6e-3, 5e-3, 9e-3), velocity=0.02,
                           travel_axis=1, depth_axis=2)
    assert (big.sample(grid, 1e-3)[mask] > 0).all()
    X = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, 300.0, material_map=mm, S=hip.MapSource(mm, big)))
    F = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, 300.0, material_map=mm, S=big.sample_device(grid, 1e-3)))
    e = rel_linf(X, F)
    print('support larger than the grid: source vs field %.2e' % e)
    assert e <= 1e-12
    plain = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, 300.0, material_map=mm))
    big.power = 0.0
    Z = np.asarray(hip.adi_step_numba_coeff(T0, grid, mm.mat, prm, mm.packs, 300.0, material_map=mm, S=hip.MapSource(mm, big)))
    assert np.array_equal(Z, plain) and not np.array_equal(X, plain)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_source_crossing_the_interface_on_512_row_lines(hip, axis):
    shape = mc.LONG[axis]
    key = ('long', shape, 'shells3', 'general' if shape[2] == 512 else 'robin_neumann', 0.5, 0.3)
    c = dict(mc.case(key))
    c['ids'] = dc.interface_ids(shape, axis=axis, copper_below=4)
    grid, mm, prm = _setup(hip, c)
    da = 2 if axis != 2 else 1
    org = [0.5 * n * c['dx'] for n in shape]
    org[da] = 0.75 * shape[da] * c['dx']
    src = hip.GoldakSource(origin=tuple(org), **dict(dc.SRC_KW, travel_axis=axis, depth_axis=da, velocity=0.0))
    q = src.sample(grid, 0.0)
    assert all(int(((q > 0) & c['mask'] & (c['ids'] == m)).sum()) >= 20 for m in (0, 2))
    X = hip.adi_step_numba_coeff(np.array(c['T0']), grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=hip.MapSource(mm, src))
    ref = mc.reference_of(c, S=dc.source_field_ld(src, shape, c['dx'], c['mask'], 0.5 * prm.dt))
    _hold(X, c, ref, 'MapSource on %d x %d x %d' % shape)


def test_graph_replay_is_the_step_loop(hip):
    c = _src_case(key=('holes', mc.HOLES, 'random3', 'general', 1.0, 0.3))
    grid, mm, prm = _setup(hip, c)
    src = _src(hip, ORIGIN)
    msrc = hip.MapSource(mm, src)
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, source=msrc)

    def six(t0):
        T = hip.to_device(c['T0'])
        for i in range(6):
            T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=msrc, t=t0 + i * prm.dt)
        return T.get()
    assert np.array_equal(st.run(hip.to_device(c['T0']), 6, t0=T_SRC).get(), six(T_SRC)) and st.captures == 1
    plain = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm).run(hip.to_device(c['T0']), 6).get()
    assert not np.array_equal(plain, six(T_SRC))
    prm.dt = 0.37 * c['dt']                                # a new dt: one recapture
    assert np.array_equal(st.run(hip.to_device(c['T0']), 6, t0=T_SRC).get(), six(T_SRC)) and st.captures == 2
    a = st.run(hip.to_device(c['T0']), 6, t0=0.4).get()    # a new t0: the block is rewritten, nothing recaptures
    assert np.array_equal(a, six(0.4)) and st.captures == 2 and not np.array_equal(a, six(T_SRC))
    assert np.array_equal(st.run(hip.to_device(c['T0']), 6, t0=0.4, graph=False).get(), a)


def test_graph_replay_with_loss_phase_and_the_recorders(hip):
    import matmap_extras_cases as xc                       # noqa: F401  (the laws' home; the figures here are this test's own)
    c = _src_case(key=('holes', mc.HOLES, 'random3', 'general', 1.0, 0.3))
    c['robin_h'] = None
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    mm = hip.MaterialMap(grid, c['materials'], np.array(c['ids']), **mc.bc_of(c))
    prm = hip.Params(c['dt'], c['theta'])
    src = _src(hip, ORIGIN, power=6000.0)
    msrc = hip.MapSource(mm, src)
    laws = (hip.PhaseChange(2.7e5, 1400.0, 1450.0), None, hip.PhaseChange(1.1e5, 900.0, 960.0))
    losses = (hip.SurfaceLoss(h=30.0, emissivity=0.4), hip.SurfaceLoss(h=80.0), hip.SurfaceLoss(h=10.0, emissivity=0.8))
    lv = hip.HistoryLevels(800.0, 500.0, 1400.0)

    def parts():
        T = hip.to_device(c['T0'])
        return T, dict(surface_loss=hip.MapLossPacks(mm, losses, c['Tinf']), phase=hip.MapPhaseField(mm, laws, T=T),
                       history=hip.ThermalHistory(grid, lv, capacity=8, T=T), solidification=hip.SolidificationRecord(grid, 1000.0, T=T),
                       monitor=hip.FieldMonitor(grid, probes=[(9, 9, 30), (12, 9, 30)], capacity=8, material_map=mm))
    T, kw = parts()
    for i in range(6):
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, S=msrc, t=T_SRC + i * prm.dt, **kw)
    T2, kw2 = parts()
    st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, c['Tinf'], material_map=mm, source=msrc, **kw2)
    got = st.run(T2, 6, t0=T_SRC)
    assert st.captures == 1 and np.array_equal(got.get(), T.get())
    assert np.array_equal(np.asarray(kw2['phase'].liquid_fraction), np.asarray(kw['phase'].liquid_fraction))
    assert np.array_equal(np.asarray(kw2['history'].T_peak), np.asarray(kw['history'].T_peak), equal_nan=True)
    assert np.array_equal(np.asarray(kw2['solidification'].t_solid), np.asarray(kw['solidification'].t_solid), equal_nan=True)
    a, b = kw2['monitor'].traces(), kw['monitor'].traces()
    assert len(a['t']) == 6
    assert np.array_equal(a['T'], b['T'], equal_nan=True)
    # (the clocks: run() forms t0 + n dt, the step loop adds dt n times -- a rounding per step apart at most)
    assert np.allclose(a['t'], b['t'], rtol=6 * mc.EPS64, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------- 4. drivers
def _same(a, b, what='result'):
    if isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], '%s[%s]' % (what, k))
    elif isinstance(a, (list, tuple)) and not np.isscalar(a):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (what, i))
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


ROBIN_H = {f: dc.H for f in dc.ROBIN}


def test_run_path_deposition_with_a_map_by_hand_and_against_the_definition(hip):
    from adi_thermal_fields_amd import waam
    path, bead, plate, dt, steps = dc.raster()
    ids = dc.plate_ids(plate)
    mmd = dict(materials=dc.MATERIALS, ids=ids, wire=dc.WIRE)
    got_T, got_mask, n = waam.run_path_deposition(hip, plate, path, bead, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt, material_map=mmd)
    grid = hip.Grid3D(*dc.SHAPE, DX, plate)
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=ROBIN_H)
    prm = hip.Params(dt, dc.THETA)
    T = hip.to_device(np.full(dc.SHAPE, dc.TINF))
    dep = hip.PathDeposit(grid, path.on_device(), bead, TS, material_map=mm, material_id=dc.WIRE)
    for t, d in steps:
        rng = dep.deposit(T, t, d)
        if rng is not None:
            mm.update(*rng)
        prm.dt = d
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, Tinf=dc.TINF, S=None, t=t, material_map=mm)
    assert n == 12
    _same((got_T, got_mask), (np.asarray(T), _mask_of(grid)))
    Td, maskd, idsd = dc.definition_loop(path, bead, plate, ids, dc.MATERIALS, dc.WIRE, steps, DX, dc.TINF, TS, dc.THETA, ROBIN_H)
    np.testing.assert_array_equal(got_mask, maskd)
    np.testing.assert_array_equal(mm.ids, idsd)
    assert maskd.sum() > plate.sum() and (idsd[maskd & ~plate] == dc.WIRE).all()
    err = rel_linf(got_T, Td)
    print('run_path_deposition(material_map=) vs the NumPy definition loop: %.2e' % err)
    assert err <= 1e-10
    with pytest.raises(ValueError, match='material_law'):
        waam.run_single_track(hip, plate, (10, 14, 4, 6, 2), DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, 1e-3, 1e-2,
                              material_map=dict(materials=dc.MATERIALS, ids=ids), material_law=object())
    with pytest.raises(ValueError, match='material_map must be a dict'):
        waam.run_path_deposition(hip, plate, path, bead, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt,
                                 material_map=dict(materials=dc.MATERIALS, ids=ids))


def test_run_path_deposition_heated_with_loss_phase_and_a_monitor_by_hand(hip):
    from adi_thermal_fields_amd import waam
    path, bead, plate, dt, steps = dc.raster()
    ids = dc.plate_ids(plate)
    laws = (hip.PhaseChange(2.7e5, 1650.0, 1720.0), hip.PhaseChange(2.0e5, 1300.0, 1360.0), None)
    losses = (hip.SurfaceLoss(h=30.0, emissivity=0.4), hip.SurfaceLoss(h=80.0), hip.SurfaceLoss(h=10.0, emissivity=0.8))
    mon = dict(probes=[(11, 6, 4), (5, 10, 5)], regions=[((0, 24), (0, 20), (0, 4)), ((0, 24), (0, 20), (4, 12))])
    got = waam.run_path_deposition(hip, plate, path, bead, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt, heat=True,
                                   surface_loss=losses, phase_change=laws, monitor=mon,
                                   material_map=dict(materials=dc.MATERIALS, ids=ids, wire=dc.WIRE))
    assert len(got) == 6
    grid = hip.Grid3D(*dc.SHAPE, DX, plate)
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=None)
    lp = hip.MapLossPacks(mm, losses, dc.TINF)
    prm = hip.Params(dt, dc.THETA)
    T = hip.to_device(np.full(dc.SHAPE, dc.TINF))
    src = path.on_device()
    dep = hip.PathDeposit(grid, src, bead, TS, material_map=mm, material_id=dc.WIRE)
    ph = hip.MapPhaseField(mm, laws, T=T)
    fm = hip.FieldMonitor(grid, t=path.t_start, capacity=len(steps), material_map=mm, **mon)
    for t, d in steps:
        rng = dep.deposit(T, t, d)
        if rng is not None:
            mm.update(*rng)
            ph.sync_mask(T)
        prm.dt = d
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, Tinf=dc.TINF, S=src.sample_step_device(grid, t, d), t=t,
                                     surface_loss=lp, phase=ph, monitor=fm, material_map=mm)
    want = (np.asarray(T), _mask_of(grid), len(steps), np.asarray(ph.liquid_fraction)) + waam.monitor_result(fm, mm.mat)
    _same(got, want)
    assert want[3].max() > 0.0 and 'heat' in want[5]


def _two_material_part():
    """a plate of STEEL (planes 0 - 3) and a block of INSULATOR on it (planes 4 - 11); COPPER's id wherever nothing is ever born"""
    full = np.zeros(dc.SHAPE, bool)
    full[:, :, :4] = True
    full[6:18, 5:15, 4:] = True
    ids = np.ones(dc.SHAPE, np.uint8)
    ids[:, :, :4] = 0
    ids[6:18, 5:15, 4:] = 2
    return full, ids


def test_run_layer_birth_with_a_map_is_the_sequence_by_hand(hip):
    import math
    import torch
    from adi_thermal_fields_amd import waam
    full, ids = _two_material_part()
    layers = waam.plan_layers(full, 2)
    tb, tout, cfl = [0.0, 0.02, 0.04, 0.2, 0.23, 0.26], [0.3], 1.0
    assert len(layers) == len(tb)
    got_T, n = waam.run_layer_birth(hip, full, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, cfl, layers, tb, tout,
                                    material_map=dict(materials=dc.MATERIALS, ids=ids))
    dt_cap = cfl * DX * DX / mc.ALPHA_MAX
    grid = hip.Grid3D(*dc.SHAPE, DX, np.zeros(dc.SHAPE, bool))
    T = hip.to_device(np.full(dc.SHAPE, dc.TINF))
    d_full = grid.layout.to_layout(full, torch.uint8)
    d_act = grid.layout.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=ROBIN_H)
    prm = hip.Params(1e-3, dc.THETA)
    steps, graphed = 0, 0
    for what, arg in waam.layer_birth_schedule(tb, tout):
        if what == 'advance':
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm.dt = max(arg / nsub, 1e-15)
            if nsub >= waam.GRAPH_MIN_NSUB:
                T = hip.StagedStepper(grid, mm.mat, prm, mm.packs, dc.TINF, material_map=mm).run(T, nsub)
                graphed += 1
            else:
                for _ in range(nsub):
                    T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, Tinf=dc.TINF, material_map=mm)
            steps += nsub
        elif what == 'birth':
            ks, ke = layers[arg]
            hip.birth_planes(T, d_act, d_full, grid, ks, ke + 1, TS)
            grid.set_mask_device(d_act, max(ks - 1, 0), min(dc.SHAPE[2], ke + 2), all_solid=False)
            mm.update(ks - 1, ke + 2)
    assert graphed >= 1 and n == steps
    _same(got_T, np.asarray(T))
    np.testing.assert_array_equal(_mask_of(grid), full)


@pytest.mark.parametrize('n_sub', [10, 16], ids=['below_GRAPH_MIN_NSUB', 'at_GRAPH_MIN_NSUB'])
def test_run_single_track_with_a_map_and_a_heat_source_is_the_sequence_by_hand(hip, n_sub):
    import torch
    from adi_thermal_fields_amd import waam
    assert waam.GRAPH_MIN_NSUB == 16
    plate = np.zeros(dc.SHAPE, bool)
    plate[:, :, :4] = True
    box = (10, 14, 4, 6, 3)
    x0, x1, z0, z1, ncol = box
    ids = np.ones(dc.SHAPE, np.uint8)
    ids[plate] = 0
    ids[x0:x1, :ncol, z0:z1] = 2
    t_step = 0.01
    dt = t_step / n_sub
    hs = hip.GoldakSource(power=600.0, eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
    got = waam.run_single_track(hip, plate, box, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt, t_step, heat_source=hs,
                                material_map=dict(materials=dc.MATERIALS, ids=ids))
    grid = hip.Grid3D(*dc.SHAPE, DX, plate.copy())
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h=ROBIN_H)
    d_mask = grid.layout.to_layout(plate, torch.uint8)
    prm = hip.Params(dt, dc.THETA)
    T = hip.to_device(np.full(dc.SHAPE, dc.TINF))
    captures = 0
    for yi in range(ncol):
        d_mask[x0:x1, yi:yi + 1, z0:z1] = 1
        grid.set_mask_device(d_mask)
        mm.rebuild()
        T[x0:x1, yi:yi + 1, z0:z1] = TS
        prm.dt = t_step / n_sub
        src = hip.MapSource(mm, waam.track_source(hs, box, DX, yi, t_step))
        if n_sub >= waam.GRAPH_MIN_NSUB:
            st = hip.StagedStepper(grid, mm.mat, prm, mm.packs, dc.TINF, source=src, material_map=mm)
            T = st.run(T, n_sub, t0=0.0)
            captures += st.captures
        else:
            for i in range(n_sub):
                T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, Tinf=dc.TINF, S=src, t=i * prm.dt, material_map=mm)
    assert captures == (ncol if n_sub >= 16 else 0)
    _same(got, np.asarray(T))
    cold = waam.run_single_track(hip, plate, box, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt, t_step,
                                 material_map=dict(materials=dc.MATERIALS, ids=ids))
    assert np.asarray(got).max() > np.asarray(cold).max()                          # the source matters


def test_one_material_and_all_ids_zero_reproduce_the_plain_drivers(hip):
    """the bar of test_matmap_gpu.py's map-against-plain test, twice bar(f, A_MAP) = 2 (A_MAP eps64 max|T| + 1e-10 inc) for one
    step, taken n times for n steps (errors add up at most linearly), with inc <= TS - TINF, the largest change a step can make"""
    from adi_thermal_fields_amd import waam
    path, bead, plate, dt, steps = dc.raster()
    one = dict(materials=[mc.STEEL], ids=np.zeros(dc.SHAPE, np.uint8))

    def hold(a, b, n, what):
        d = float(np.max(np.abs(np.asarray(a) - np.asarray(b))))
        bar = 2 * n * (mc.A_MAP * mc.EPS64 * float(np.max(np.abs(b))) + 1e-10 * (TS - dc.TINF))
        print('%-40s map vs plain %.2e K, bar %.2e K (%d steps)' % (what, d, bar, n))
        assert d <= bar
    a = waam.run_path_deposition(hip, plate, path, bead, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt, material_map=dict(one, wire=0))
    b = waam.run_path_deposition(hip, plate, path, bead, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt)
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2] == 12
    hold(a[0], b[0], 12, 'run_path_deposition')
    full, _ = _two_material_part()
    layers = waam.plan_layers(full, 2)
    tb, tout = [0.0, 0.02, 0.04, 0.2, 0.23, 0.26], [0.3]
    cfl = 0.2
    a = waam.run_layer_birth(hip, full, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, cfl, layers, tb, tout, material_map=one)
    b = waam.run_layer_birth(hip, full, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, cfl, layers, tb, tout)
    assert a[1] == b[1]
    hold(a[0], b[0], a[1], 'run_layer_birth')
    box = (10, 14, 4, 6, 3)
    hs = hip.GoldakSource(power=600.0, eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
    a = waam.run_single_track(hip, plate, box, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, 1e-3, 0.01, heat_source=hs, material_map=one)
    b = waam.run_single_track(hip, plate, box, DX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, 1e-3, 0.01, heat_source=hs)
    hold(a, b, 30, 'run_single_track')
