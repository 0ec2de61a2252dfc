"""CPU: births along a scan path (include/adi_hip.h, "Bead deposition along a scan path") -- the library's host evaluator and
index box against the NumPy definition PathDeposit.reference on the shared cases (bead_cases.py), the partition property, a
closed form, and the argument checks, which all run before any HIP call.  No GPU."""
import ctypes

import numpy as np
import pytest

import bead_cases as bc
from bead_cases import CASES, DX, TS, HostGrid

from adi_thermal_fields_amd import _lib
from adi_thermal_fields_amd.heat_source import ScanPath
from adi_thermal_fields_amd.deposition import BeadProfile, PathDeposit

IDS = [c.name for c in CASES]


def _deposit(case, mask):
    return PathDeposit(HostGrid(case.shape, DX, mask), case.path, case.bead, TS, within=case.within)


def _raw_box(dep, shape, t, dt):
    """adi_bead_index_box itself: (slices, deposits)"""
    box, flag = (ctypes.c_int * 6)(), ctypes.c_int(-1)
    _lib.check(_lib.lib.adi_bead_index_box(*dep._path_args(), *shape, DX, float(t), float(dt), box, ctypes.byref(flag)))
    return tuple(slice(box[2 * a], box[2 * a + 1]) for a in range(3)), flag.value


def _has_piece(path, bead, shape, t, dt):
    return any(True for _ in PathDeposit.reference_terms(path, bead, shape, DX, t, dt))


# ------------------------------------------------------------------------------------------- the evaluator is the definition
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_host_evaluator_equals_reference(case):
    """array for array, window after window on the growing mask; and over the whole path"""
    mask = case.active.copy()
    dep = _deposit(case, mask)
    total = 0
    for t, dt in case.windows:
        want = case.reference(t, dt, active=mask)
        np.testing.assert_array_equal(dep.born_host(t, dt), want)
        assert not (want & mask).any()
        mask |= want
        total += int(want.sum())
    t, dt = case.whole()
    mask[...] = case.active
    want = case.reference(t, dt)
    np.testing.assert_array_equal(dep.born_host(t, dt), want)
    nothing = case.name in ('jump_step_inside_the_jump', 'jump_before_t_start', 'jump_after_t_end', 'wholly_outside')
    assert (total == 0) == nothing, total
    if case.name != 'wholly_outside':
        assert want.any()


def test_the_cases_cover_what_they_claim():
    by = bc.BY_NAME
    assert {c.da for c in CASES} == {0, 1, 2} and {c.bead.profile for c in CASES} == {'box', 'parabola'}
    assert any(c.within is not None for c in CASES) and any(c.within is None for c in CASES)
    # part of the bead is active already / cut off by `within`
    for name in ('leg_plus_v', 'jump_whole', 'out_v_high'):
        c = by[name]
        free = PathDeposit.reference(c.path, c.bead, c.shape, DX, *c.whole(), within=c.within)
        assert (free & c.active).any() and (free & ~c.active).any(), name
    for name in ('oblique', 'out_v_low'):
        c = by[name]
        free = PathDeposit.reference(c.path, c.bead, c.shape, DX, *c.whole())
        assert (free & ~c.within).any() and (free & c.within).any(), name
    # one step over three segments, one of them a jump
    c = by['jump_three_segments_one_step']
    t, dt = c.windows[0]
    tab = c.path.table()
    assert t < tab[1, 0] and t + dt > tab[2, 0] and tab[1, 7] == 0.0
    # the lateral sides, the bottom and the top
    for name, ax, side in (('out_u_low', 0, 0), ('out_u_high', 0, -1), ('out_v_low', 1, 0), ('out_v_high', 1, -1)):
        c = by[name]
        born = PathDeposit.reference(c.path, c.bead, c.shape, DX, *c.whole())
        assert np.take(born, side, axis=ax).any(), name
    assert PathDeposit.reference(by['below_plane_0'].path, by['below_plane_0'].bead, bc.SHAPES[0], DX, *by['below_plane_0'].whole())[:, :, 0].any()
    top = PathDeposit.reference(by['above_the_top'].path, by['above_the_top'].bead, bc.SHAPES[0], DX, *by['above_the_top'].whole())
    assert top[:, :, -1].any() and not top[:, :, :-1].any()


# ------------------------------------------------------------------------------------------------------------ the index box
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_index_box_holds_every_born_cell(case):
    dep = _deposit(case, np.zeros(case.shape, dtype=bool))
    for t, dt in list(case.windows) + [case.whole()]:
        born = PathDeposit.reference(case.path, case.bead, case.shape, DX, t, dt)
        box, flag = _raw_box(dep, case.shape, t, dt)
        outside = born.copy()
        outside[box] = False
        assert not outside.any(), (t, dt)
        assert flag == int(_has_piece(case.path, case.bead, case.shape, t, dt))
        if not flag:
            assert all(s.start == 0 and s.stop == 0 for s in box)
        got = dep.index_box(t, dt)
        assert (got is None) == (not flag or any(s.start >= s.stop for s in box))
        if got is not None:
            assert got == tuple((s.start, s.stop) for s in box)


def test_index_box_on_random_paths():
    """200 seeded paths of two to five segments -- legs, jumps, dwells with and without power -- in and around a 13 x 11 x 9 grid"""
    rng = np.random.default_rng(20240611)
    shape = bc.SHAPES[1]
    n_dep = n_none = n_born = 0
    for _ in range(200):
        da = int(rng.integers(0, 3))
        au, av = bc.axes_of(da)
        lo, hi = np.array([-4.0, -4.0]), np.array([shape[au] + 4.0, shape[av] + 4.0])
        z = rng.uniform(-1.0, shape[da] + 3.0)
        pt = lambda: bc.point(da, *(rng.uniform(lo, hi) * DX), z * DX)          # noqa: E731
        path = ScanPath(power=500.0, depth_axis=da, start=pt(), t_start=rng.uniform(-1.0, 1.0), **bc.GOLDAK)
        for _s in range(int(rng.integers(2, 6))):
            kind = rng.random()
            if kind < 0.15:
                path.dwell(rng.uniform(0.05, 0.4), power=float(rng.choice([0.0, 300.0])))
            else:
                path.line_to(pt(), rng.uniform(5.0, 40.0) * DX, power=0.0 if kind < 0.35 else None)
        bead = BeadProfile(rng.uniform(0.6, 6.0) * DX, rng.uniform(0.6, 5.0) * DX, str(rng.choice(['box', 'parabola'])))
        dep = PathDeposit(HostGrid(shape, DX, np.zeros(shape, dtype=bool)), path, bead, TS)
        t = rng.uniform(path.t_start - 0.3, path.t_end)
        dt = rng.uniform(0.01, 1.2) * (path.t_end - path.t_start)
        born = PathDeposit.reference(path, bead, shape, DX, t, dt)
        box, flag = _raw_box(dep, shape, t, dt)
        outside = born.copy()
        outside[box] = False
        assert not outside.any()
        assert flag == int(_has_piece(path, bead, shape, t, dt))
        n_dep += flag
        n_none += not flag
        n_born += bool(born.any())
    assert n_dep >= 100 and n_none >= 5 and n_born >= 50, (n_dep, n_none, n_born)


# ------------------------------------------------------------------------------------------------------- partition property
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_partition_property_host(case):
    """the OR of the births over the steps of a partition is the births of one step over the whole interval, exactly"""
    mask = case.active.copy()
    dep = _deposit(case, mask)
    whole = dep.born_host(*case.whole())
    np.testing.assert_array_equal(whole, case.reference(*case.whole()))
    for f in bc.PARTITION_FACTORS:
        dt = f * case.path.t_end / 5
        acc = np.zeros(case.shape, dtype=bool)
        t = case.path.t_start
        while t < case.path.t_end:
            acc |= dep.born_host(t, dt)
            t = t + dt
        np.testing.assert_array_equal(acc, whole, err_msg='dt = %g t_end / 5' % f)


# -------------------------------------------------------------------------------------------------------------- closed form
@pytest.mark.parametrize('da', [2, 0])
def test_closed_form_block(da):
    """a box bead along +axis 1 of width m dx centred on a cell face and height n dx with its top on a cell face: every row whose
    centre projects inside the leg is exactly the m x n block of cells"""
    shape = (16, 20, 12)
    m, n = 4, 3
    # depth axis 2: the leg runs along axis 1 (the second in-plane axis) at u = 7 dx, top at 9 dx; depth axis 0: along axis 1
    # (the first in-plane axis) at v = 6 dx, top at 11 dx
    if da == 2:
        p0, p1, cross_axis, c, top = (7.0, 3.0, 9.0), (7.0, 15.0, 9.0), 0, 7, 9
    else:
        p0, p1, cross_axis, c, top = (11.0, 3.0, 6.0), (11.0, 15.0, 6.0), 2, 6, 11
    path = ScanPath(power=800.0, depth_axis=da, start=tuple(v * DX for v in p0), **bc.GOLDAK).line_to(tuple(v * DX for v in p1), 10 * DX)
    bead = BeadProfile(m * DX, n * DX, 'box')
    for _, r2, h2, z, cap in PathDeposit.reference_terms(path, bead, shape, DX, -1.0, 5.0):
        assert min(np.abs(r2 - h2).min() / h2, np.abs(-z - cap).min() / (n * DX), np.abs(z).min() / DX) >= bc.MARGIN
    dep = PathDeposit(HostGrid(shape, DX, np.zeros(shape, dtype=bool)), path, bead, TS)
    born = dep.born_host(-1.0, 5.0)
    np.testing.assert_array_equal(born, PathDeposit.reference(path, bead, shape, DX, -1.0, 5.0))
    block = np.zeros(shape, dtype=bool)
    sl = [slice(None)] * 3
    sl[cross_axis], sl[da] = slice(c - m // 2, c + m // 2), slice(top - n, top)
    block[tuple(sl)] = True
    rows = [j for j in range(shape[1]) if 3.0 < j + 0.5 < 15.0]             # centres that project inside the leg
    assert len(rows) == 12
    for j in rows:
        np.testing.assert_array_equal(born[:, j, :], block[:, j, :], err_msg='row %d' % j)
    assert born[:, rows, :].sum() == len(rows) * m * n
    # beyond the ends the round caps hold less than the block, and nothing lies further than width / 2 from them
    assert 0 < born[:, 1, :].sum() < m * n and not born[:, 0, :].any() and not born[:, 17:, :].any()


# ------------------------------------------------------------------------------------------------------- argument errors
def test_bead_profile_errors():
    for w, h, p, msg in ((0.0, 1e-3, 'box', 'non-positive'), (-1e-3, 1e-3, 'box', 'non-positive'), (1e-3, 0.0, 'box', 'non-positive'),
                         (np.inf, 1e-3, 'box', 'non-finite'), (1e-3, np.nan, 'box', 'non-finite'), ('wide', 1e-3, 'box', 'real numbers'),
                         (1e-3, 1e-3, 'round', 'profile'), (1e-3, 1e-3, 1, 'profile')):
        with pytest.raises(ValueError, match='BeadProfile: .*%s' % msg):
            BeadProfile(w, h, p)
    with pytest.raises(TypeError, match='BeadProfile'):
        PathDeposit(HostGrid((4, 4, 4), DX, np.zeros((4, 4, 4), bool)), CASES[0].path, (1e-3, 1e-3), TS)
    with pytest.raises(TypeError, match='ScanPath'):
        PathDeposit(HostGrid((4, 4, 4), DX, np.zeros((4, 4, 4), bool)), 'path', BeadProfile(1e-3, 1e-3), TS)
    with pytest.raises(ValueError, match='non-finite Ts'):
        PathDeposit(HostGrid((4, 4, 4), DX, np.zeros((4, 4, 4), bool)), CASES[0].path, BeadProfile(1e-3, 1e-3), np.nan)
    with pytest.raises(ValueError, match='within has shape'):
        PathDeposit(HostGrid((4, 4, 4), DX, np.zeros((4, 4, 4), bool)), CASES[0].path, BeadProfile(1e-3, 1e-3), TS,
                    within=np.ones((4, 4, 5), bool))


def test_library_argument_errors_come_before_any_hip_call():
    """every entry refuses a bad argument with ADI_ERR_ARG (a ValueError) on a box without a GPU: the device entry too, handed
    pointers it must never follow"""
    L = _lib.lib
    case = CASES[0]
    tab = np.ascontiguousarray(case.path.table())
    K, t_end = tab.shape[0], case.path.t_end
    good = _lib.BeadShape(3e-3, 2e-3, 0, 2)
    born = np.zeros((4, 4, 4), dtype=np.uint8)
    P = ctypes.c_void_p
    fake, fake2 = P(4096), P(8192)

    def host(shape=good, table=tab, K=K, t_end=t_end, t=0.0, dt=0.5):
        _lib.check(L.adi_bead_deposit_host(ctypes.byref(shape), table.ctypes.data, K, t_end, None, None, 4, 4, 4, DX, t, dt,
                                           born.ctypes.data))

    def box(shape=good, table=tab, t=0.0, dt=0.5):
        b, f = (ctypes.c_int * 6)(), ctypes.c_int()
        _lib.check(L.adi_bead_index_box(ctypes.byref(shape), table.ctypes.data, K, t_end, 4, 4, 4, DX, t, dt, b, ctypes.byref(f)))

    def dev(shape=good, table=tab, t=0.0, dt=0.5, Ts=TS, l=(4, 4, 4), n=(4, 4, 4), active=fake, within=None):
        _lib.check(L.adi_bead_deposit(ctypes.byref(shape), table.ctypes.data, fake2, K, t_end, fake2, active, within, *l, *n, 0,
                                      DX, t, dt, Ts, fake2, None))
    host()                                                                  # (the arguments the others are varied from)
    box()
    for fn in (host, box, dev):
        for bad, msg in ((_lib.BeadShape(0.0, 2e-3, 0, 2), 'width'), (_lib.BeadShape(3e-3, -1.0, 0, 2), 'height'),
                         (_lib.BeadShape(np.inf, 2e-3, 0, 2), 'non-finite'), (_lib.BeadShape(3e-3, 2e-3, 2, 2), 'profile'),
                         (_lib.BeadShape(3e-3, 2e-3, 0, 3), 'depth_axis')):
            with pytest.raises(ValueError, match=msg):
                fn(shape=bad)
        with pytest.raises(ValueError, match='dt must be > 0'):
            fn(dt=0.0)
        with pytest.raises(ValueError, match='dt must be > 0'):
            fn(dt=-0.1)
        with pytest.raises(ValueError, match='bad t / dt'):
            fn(t=np.nan)
        desc = tab.copy()
        desc[0, 0] = desc[-1, 0] + 1.0 if K > 1 else t_end + 1.0
        with pytest.raises(ValueError, match='does not ascend|not after the last'):
            fn(table=desc)
        notunit = tab.copy()
        notunit[0, 4] = 0.5
        with pytest.raises(ValueError, match='unit vector'):
            fn(table=notunit)
    two = np.ascontiguousarray(bc.BY_NAME['corner'].path.table())
    two[1, 0] = two[0, 0] - 0.1                                             # descending t_begin in a table of two segments
    with pytest.raises(ValueError, match='t_begin does not ascend'):
        _lib.check(L.adi_bead_deposit(ctypes.byref(good), two.ctypes.data, fake2, 2, 9.0, fake2, fake, None, 4, 4, 4, 4, 4, 4, 0, DX, 0.0,
                                      0.5, TS, fake2, None))
    with pytest.raises(ValueError, match='non-finite Ts'):
        dev(Ts=np.inf)
    with pytest.raises(ValueError, match='non-finite Ts'):
        dev(Ts=np.nan)
    with pytest.raises(ValueError, match='exceeds the physical'):
        dev(l=(5, 4, 4))
    with pytest.raises(ValueError, match='exceeds the physical'):
        dev(l=(4, 4, 9), n=(4, 4, 8))
    with pytest.raises(ValueError, match='aliases'):
        dev(within=fake)
    with pytest.raises(ValueError, match='null argument'):
        dev(active=None)
    with pytest.raises(ValueError, match='dt'):
        PathDeposit.reference(case.path, case.bead, case.shape, DX, 0.0, 0.0)
