"""GPU: births along a scan path on the device (PathDeposit.deposit, adi_bead_deposit) against the NumPy definition
PathDeposit.reference on the shared cases (bead_cases.py): mask, field (padding included), count and plane range; the rebuilt
flags, bricks and packs against a fresh grid; the partition property; and waam.run_path_deposition against the same loop on
the pinned CPU oracle and against the sequence of calls done by hand."""
import numpy as np
import pytest

import bead_cases as bc
from bead_cases import CASES, DX, TS

pytestmark = pytest.mark.gpu

RHO, CP, K = 7800.0, 500.0, 30.0
ROBIN = {'x-': 40.0, 'x+': 55.0, 'y-': 70.0, 'y+': 85.0, 'z-': 100.0, 'z+': 115.0}


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _raw(t):
    """a tensor's whole storage, padding included, as it is in memory"""
    n = t.untyped_storage().nbytes() // t.element_size()
    return t.as_strided((n,), (1,))


def _logical(layout):
    """bool over the storage of a field in `layout`: the cells of the logical box"""
    import torch
    idx = torch.zeros(layout.numel_padded, dtype=torch.bool, device='cuda')
    idx.as_strided(layout.shape, layout.strides).fill_(True)
    return idx


def _mask_of(g):
    return g.d_mask.cpu().numpy().astype(bool)


def _field(hip, g, seed):
    """a DeviceField in the grid's layout whose every byte, padding included, is random; and its logical values"""
    import torch
    rng = np.random.default_rng(seed)
    T0 = rng.uniform(300.0, 900.0, g.shape)
    t = g.layout.empty()
    _raw(t).copy_(torch.from_numpy(rng.uniform(1.0, 2.0, g.layout.numel_padded)))
    t.copy_(torch.from_numpy(T0))
    return hip.DeviceField(t), T0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _expected_range(case, box, nz):
    return (max(0, box[2][0] - 1), min(nz, box[2][1] + 1)) if case.da == 2 else (0, nz)


def _check_case(hip, case):
    import torch
    g = hip.Grid3D(*case.shape, DX, case.active)
    T, T0 = _field(hip, g, 7)
    dep = hip.PathDeposit(g, case.path, case.bead, TS, within=case.within)
    logical = _logical(g.layout)
    count = torch.full((1,), -7, dtype=torch.int64, device='cuda')
    mask = case.active.copy()
    np.testing.assert_array_equal(_mask_of(g), mask)
    for t, dt in case.windows:
        want = case.reference(t, dt, active=mask)
        before = _raw(T.t).clone()
        version, flags = g.mask_version, g.d_flags.clone()
        box = dep.index_box(t, dt)
        rng = dep.deposit(T, t, dt, count=count)
        np.testing.assert_array_equal(_mask_of(g), mask | want)
        assert int(count.item()) == int(want.sum())
        now = T.t.cpu().numpy()
        assert (now[want] == TS).all()
        np.testing.assert_array_equal(_bits(now[~want]), _bits(T0[~want]))
        assert torch.equal(_raw(T.t)[~logical], before[~logical])               # the padding of the field: every bit as it was
        assert not _raw(g.d_mask)[~logical].any()                                # ... and of the mask: still off
        if box is None:
            assert rng is None and not want.any()
            assert g.mask_version == version and torch.equal(g.d_flags, flags)
        else:
            assert rng == _expected_range(case, box, case.shape[2])
            assert g.mask_version != version
            if case.da == 2 and want.any():
                ks = np.flatnonzero(want.any(axis=(0, 1)))
                assert rng[0] <= max(0, ks[0] - 1) and rng[1] >= min(case.shape[2], ks[-1] + 2)
        mask |= want
        T0 = np.where(want, TS, T0)
    return g, T


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_deposit_equals_reference(mods, case):
    _check_case(mods[0], case)


@pytest.mark.parametrize('name,phys', [('corner', (28, 24, 16)), ('corner_depth_axis_0', (27, 23, 20)), ('above_the_top', (24, 20, 16)),
                                       ('small_oblique_depth_axis_0', (16, 13, 12))])
def test_deposit_on_a_forced_padded_box(mods, monkeypatch, name, phys):
    hip = mods[0]
    monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)
    g, _ = _check_case(hip, bc.BY_NAME[name])
    assert g.layout.padded and g.layout.pd[:3] == phys


def test_one_case_runs_on_a_box_the_library_pads(mods):
    """(test_deposit_equals_reference[padded_by_the_library] compares that padding too)"""
    hip = mods[0]
    assert hip.Layout(*bc.PADDED_SHAPE).padded and bc.BY_NAME['padded_by_the_library'].shape == bc.PADDED_SHAPE


# --------------------------------------------------------------------------------------------- flags, bricks and packs
@pytest.mark.parametrize('name', ['below_plane_0', 'top_plane', 'above_the_top', 'corner_depth_axis_0', 'jump_whole', 'ragged_raster',
                                  'padded_by_the_library'])
def test_rebuilt_flags_bricks_and_packs_equal_a_fresh_build(mods, name):
    """beads at k = 0, at k = nz - 1 and along another depth axis: after deposit and BirthPacks.update on the range it returns,
    every array the step reads is what a grid built from the downloaded mask holds"""
    import torch
    hip = mods[0]
    case = bc.BY_NAME[name]
    nz = case.shape[2]
    g = hip.Grid3D(*case.shape, DX, case.active)
    mat = hip.Material(RHO, CP, K)
    T, _ = _field(hip, g, 11)
    dep = hip.PathDeposit(g, case.path, case.bead, TS, within=case.within)
    bp = hip.BirthPacks(g, mat, robin_h=ROBIN)
    born_planes = np.zeros(nz, dtype=bool)
    for t, dt in list(case.windows) + [case.whole()]:
        before = _mask_of(g)
        rng = dep.deposit(T, t, dt)
        born_planes |= (_mask_of(g) & ~before).any(axis=(0, 1))
        if rng is not None:
            bp.update(*rng)
    assert born_planes.any()
    if name == 'below_plane_0':
        assert born_planes[0]
    if name in ('top_plane', 'above_the_top'):
        assert born_planes[nz - 1]
    fresh = hip.Grid3D(*case.shape, DX, _mask_of(g))
    fp = hip.BirthPacks(fresh, mat, robin_h=ROBIN)
    assert torch.equal(_raw(g.d_flags), _raw(fresh.d_flags))
    assert torch.equal(g.d_bricks, fresh.d_bricks)
    for a in range(3):
        assert torch.equal(_raw(bp.coeff[a]).view(torch.int64), _raw(fp.coeff[a]).view(torch.int64)), a
        assert torch.equal(_raw(bp.qflux[a]).view(torch.int64), _raw(fp.qflux[a]).view(torch.int64)), a
        assert bp.packs[a].mask_version == g.mask_version


# ----------------------------------------------------------------------------------------------------- partition property
@pytest.mark.parametrize('name', ['jump_whole', 'corner_parabola_within', 'jump_depth_axis_1', 'oblique_leaves_the_corner',
                                  'ragged_raster'])
def test_partition_property_device(mods, name):
    hip = mods[0]
    case = bc.BY_NAME[name]
    whole = case.active | case.reference(*case.whole())
    for f in bc.PARTITION_FACTORS:
        g = hip.Grid3D(*case.shape, DX, case.active)
        T, T0 = _field(hip, g, 3)
        dep = hip.PathDeposit(g, case.path, case.bead, TS, within=case.within)
        dt = f * case.path.t_end / 5
        t = case.path.t_start
        while t < case.path.t_end:
            dep.deposit(T, t, dt)
            t = t + dt
        np.testing.assert_array_equal(_mask_of(g), whole, err_msg='dt = %g t_end / 5' % f)
        born = whole & ~case.active
        now = T.t.cpu().numpy()
        assert (now[born] == TS).all()
        np.testing.assert_array_equal(_bits(now[~born]), _bits(T0[~born]))


# --------------------------------------------------------------------------------------------------------------- the driver
SHAPE = bc.SHAPES[0]
TINF, THETA = 300.0, 0.5
H = 35.0


def _raster():
    """two beads on a plate of 4 planes: a leg, a jump, the leg back; the bead fills planes 4 and 5"""
    from adi_thermal_fields_amd.heat_source import ScanPath
    from adi_thermal_fields_amd.deposition import BeadProfile, PathDeposit
    top = 6.3
    P = lambda u, v: (u * DX, v * DX, top * DX)                                  # noqa: E731
    path = ScanPath(power=200.0, start=P(4.37, 6.21), t_start=0.125, **bc.GOLDAK)
    path.line_to(P(18.13, 6.21), 40 * DX).line_to(P(18.13, 10.47), 120 * DX, power=0.0).line_to(P(4.37, 10.47), 40 * DX)
    bead = BeadProfile(3.3 * DX, 2.4 * DX, 'parabola')
    plate = np.zeros(SHAPE, dtype=bool)
    plate[:, :, :4] = True
    dt = (path.t_end - path.t_start) / 11.5                                      # 12 steps, the last one half as long
    steps = []
    t = path.t_start
    while t < path.t_end:
        d = dt if t + dt <= path.t_end else path.t_end - t
        steps.append((t, d))
        t = t + d
    assert len(steps) == 12 and steps[-1][1] < 0.6 * dt
    for t, d in steps:                                                           # the inputs keep their margin in every step
        for _, r2, h2, z, cap in PathDeposit.reference_terms(path, bead, SHAPE, DX, t, d):
            assert min(np.abs(r2 - h2).min() / h2, np.abs(-z - cap).min() / (2.4 * DX), np.abs(z).min() / DX) >= bc.MARGIN
    return path, bead, plate, dt, steps


@pytest.mark.parametrize('heat', [False, True], ids=['births_only', 'heated_by_the_path'])
def test_run_path_deposition_vs_oracle(mods, heat):
    """the driver against the same loop on the CPU oracle: births by PathDeposit.reference, packs rebuilt in full after every
    step's births, the heat input as the host field ScanPath.sample_step folded into the axis-0 pack"""
    from adi_thermal_fields_amd import waam
    from adi_thermal_fields_amd.deposition import PathDeposit
    hip, orc = mods
    path, bead, plate, dt, steps = _raster()
    got_T, got_mask, n = waam.run_path_deposition(hip, plate, path, bead, DX, (RHO, CP, K), H, TINF, TS, THETA, dt, heat=heat)
    mask = plate.copy()
    T = np.full(SHAPE, TINF)
    mat, prm = orc.Material(RHO, CP, K), orc.Params(dt, THETA)
    robin = {f: H for f in ROBIN}
    for t, d in steps:
        born = PathDeposit.reference(path, bead, SHAPE, DX, t, d, active=mask)
        T[born] = TS
        mask |= born
        go = orc.Grid3D(*SHAPE, DX, mask)
        packs = orc.precompute_coeff_packs_unified(go, mat, robin_h=robin, robin_Tinf=TINF)
        if heat:
            packs[0].qflux = packs[0].qflux + path.sample_step(go, t, d) / (RHO * CP)
        prm.dt = d
        T = orc.adi_step_numba_coeff(T, go, mat, prm, packs, Tinf=TINF)
    assert n == 12 and mask.sum() > plate.sum()
    np.testing.assert_array_equal(got_mask, mask)
    err = rel_linf(got_T, T)
    print('run_path_deposition (heat=%s) vs oracle: %.2e' % (heat, err))
    assert err <= 1e-10
    np.testing.assert_array_equal(got_T[~mask], TINF)
    if heat:
        assert T.max() > TS + 1.0                                                # the arc matters at this scale


def _same(a, b, what):
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


def test_run_path_deposition_with_extras_is_the_sequence_by_hand(mods):
    """phase change, history and solidification through the driver, against PathDeposit.deposit, BirthPacks.update, sync_mask and
    adi_step_numba_coeff called one after the other: every returned array bit for bit"""
    from adi_thermal_fields_amd import waam
    hip, _ = mods
    path, bead, plate, dt, steps = _raster()
    law = hip.PhaseChange(2.7e5, 1650.0, 1720.0)
    levels = hip.HistoryLevels(800.0, 500.0, 1700.0)
    T_freeze = 1700.0
    got = waam.run_path_deposition(hip, plate, path, bead, DX, (RHO, CP, K), H, TINF, TS, THETA, dt, heat=True, phase_change=law,
                                   history=levels, solidification=T_freeze)
    assert len(got) == 6
    grid = hip.Grid3D(*SHAPE, DX, plate)
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, THETA)
    T = hip.to_device(np.full(SHAPE, TINF))
    src = path.on_device()
    dep = hip.PathDeposit(grid, src, bead, TS)
    bp = hip.BirthPacks(grid, mat, robin_h={f: H for f in ROBIN})
    packs = bp.packs
    ph = hip.PhaseField(grid, mat, law, T=T)
    hist = hip.ThermalHistory(grid, levels, capacity=len(steps), T=T, t=path.t_start)
    sol = hip.SolidificationRecord(grid, T_freeze, T=T, t=path.t_start)
    for t, d in steps:
        rng = dep.deposit(T, t, d)
        if rng is not None:
            packs = bp.update(*rng)
            for x in (ph, hist, sol):
                x.sync_mask(T)
        prm.dt = d
        T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=TINF, S=src.sample_step_device(grid, t, d), t=t, phase=ph,
                                     history=hist, solidification=sol)
    want = (np.asarray(T), _mask_of(grid), len(steps), np.asarray(ph.liquid_fraction), waam.history_result(hist),
            waam.solidification_result(sol))
    _same(got, want, 'result')
    assert want[3].max() > 0.0 and np.isfinite(want[4]['T_peak'][want[1]]).all()


def test_no_step_before_the_first_deposit_on_an_empty_base(mods):
    """an empty base mask: the steps before the path starts to deposit are not taken"""
    from adi_thermal_fields_amd import waam
    hip, _ = mods
    path, bead, plate, dt, steps = _raster()
    empty = np.zeros(SHAPE, dtype=bool)
    late = hip.ScanPath(power=200.0, start=path.start, t_start=path.t_start, **bc.GOLDAK)
    late.dwell(3.2 * dt).line_to((18.13 * DX, 6.21 * DX, 6.3 * DX), 40 * DX)
    T, mask, n = waam.run_path_deposition(hip, empty, late, bead, DX, (RHO, CP, K), H, TINF, TS, THETA, dt)
    total = len(waam.path_steps(late.t_start, late.t_end, dt))
    assert n == total - 3 and mask.any()
    np.testing.assert_array_equal(T[~mask], TINF)
