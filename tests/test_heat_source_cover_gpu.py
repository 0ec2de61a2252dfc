"""GPU: the moving Goldak source where test_heat_source_gpu.py does not reach -- supports wider than the grid (the launch box
of k_source_lines0 / k_source_lines0_long clamped to n + 4 lines along axis 1, axis 2 or both), every (travel, depth)
orientation, every way the correction assembles A0 (lines0_row), padded layouts and line lengths at the form switches,
and the single-track driver on a plate thinner than the source's depth support.

The reference is the one of test_heat_source_gpu.py: the pinned CPU oracle with q/(rho cp) folded into the axis-0 pack's
qflux, GoldakSource.sample the ground truth for q.  The energy checks need no oracle: with adiabatic packs (no Robin, no
Neumann, no Dirichlet) and T0 = 0, rho cp dx^3 sum_mask T_N must equal sum_n dt dx^3 sum q(t_n + dt/2), so a line the
correction never visits shows up as missing energy."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_heat_source_gpu import CP, FACES, K, KAPPA, RHO, make_case, mods, oracle_step, rel_linf, setup  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DX = 1e-4
DT = 0.5 * DX * DX / KAPPA
R_CUT = np.sqrt(40.0 / 3.0)          # half-extent of the support in units of a length (E_CUT = 40)


def goldak(hip, a, b, c_f, c_r, centre, travel_axis, depth_axis, sign=1, cells_per_step=0.0, rise=20.0, t0=0.0):
    """a GoldakSource with lengths in cells, centred at `centre` (cells) at time t0, moving `cells_per_step` per DT, its
    power set for a peak of about `rise` kelvin per step"""
    L = [v * DX for v in (a, b, c_f, c_r)]
    P = rise * RHO * CP * L[0] * L[1] * L[2] * np.pi ** 1.5 / (6.0 * np.sqrt(3.0) * 0.8 * 1.2 * DT)
    v = cells_per_step * DX / DT
    origin = [c * DX for c in centre]
    origin[travel_axis] -= sign * v * t0
    return hip.GoldakSource(P, 0.8, *L, f_f=1.2, origin=tuple(origin), velocity=v, travel_axis=travel_axis,
                            travel_sign=sign, depth_axis=depth_axis)


def advance(hip, runner, g, mat, prm, packs, src, T0, nsteps, t0=0.0, Tinf=300.0, fused=None):
    """nsteps steps of the moving source from t0 through `runner`: 'func' (adi_step_numba_coeff(S=src, t=)), 'step'
    (StagedStepper.step(t=)) or 'run' (StagedStepper.run(t0=), a captured graph replayed)"""
    T = hip.to_device(T0)
    if runner == 'func':
        for n in range(nsteps):
            T = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=Tinf, S=src, t=t0 + n * prm.dt)
        return np.asarray(T)
    st = hip.StagedStepper(g, mat, prm, packs, Tinf=Tinf, fused=fused, source=src)
    if runner == 'run':
        return np.asarray(st.run(T, nsteps, t0=t0))
    for n in range(nsteps):
        T = st.step(T, t=t0 + n * prm.dt)
    return np.asarray(T)


def oracle_loop(orc, T0, go, mato, prmo, kw, src, nsteps, t0=0.0, Tinf=300.0):
    To = np.array(T0, dtype=np.float64)
    for n in range(nsteps):
        To = oracle_step(orc, To, go, mato, prmo, kw, src.sample(go, t0 + n * prmo.dt + 0.5 * prmo.dt), Tinf=Tinf)
    return To


def check_vs_oracle(hip, orc, shape, src, runner, nsteps, t0=0.0, fused=None, label=''):
    """the mixed case of make_case (holes, Dirichlet cells, Robin, Neumann) stepped with `src` against the oracle"""
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, DX, DT)
    got = advance(hip, runner, g, mat, prm, packs, src, T0, nsteps, t0=t0, fused=fused)
    want = oracle_loop(orc, T0, go, mato, prmo, kw, src, nsteps, t0=t0)
    err = rel_linf(got, want)
    print('%s vs oracle: rel_linf %.3e (%d steps)' % (label, err, nsteps))
    assert err <= (1e-12 if nsteps == 1 else 1e-10), err
    plain = orc.adi_run(T0, go, mato, prmo, orc.precompute_coeff_packs_unified(go, mato, **kw), Tinf=300.0,
                        nsteps=nsteps)
    assert np.abs(want - plain).max() > 1.0                      # the source reached the field
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])
    dm = kw['dir_mask']
    np.testing.assert_array_equal(got[dm], kw['dir_value'][dm])
    return g


def check_energy(hip, orc, shape, src, runner, nsteps, t0=0.0, fused=None, label=''):
    """adiabatic packs, T0 = 0: the field's energy is the energy the source put in"""
    mask, _, _ = make_case(shape, DX, dirichlet=False)
    g, go = hip.Grid3D(*shape, DX, mask), orc.Grid3D(*shape, DX, mask)
    mat, prm = hip.Material(RHO, CP, K), hip.Params(DT, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat)
    TN = advance(hip, runner, g, mat, prm, packs, src, np.zeros(shape), nsteps, t0=t0, Tinf=0.0, fused=fused)
    e_field = RHO * CP * DX ** 3 * TN[mask].sum()
    e_in = sum(DT * DX ** 3 * src.sample(go, t0 + n * DT + 0.5 * DT).sum() for n in range(nsteps))
    print('%s energy: field / input - 1 = %.3e' % (label, e_field / e_in - 1.0))
    assert e_in > 0
    assert abs(e_field - e_in) <= 1e-11 * e_in, (e_field, e_in)


def box_clamped(src, g, axis):
    """the launch box along `axis` (1 or 2) has more lines than the physical extent + 4 (lines0_box clamps it)"""
    ta = src.travel_axis
    if axis == ta:
        ext = R_CUT * (src.c_f + src.c_r)
    else:
        ext = 2.0 * R_CUT * (src.b if axis == src.depth_axis else src.a)
    return int(np.floor(ext / g.dx)) + 4 > g.layout.pd[axis] + 4


# Supports wider than the grid.  (shape, source (a, b, c_f, c_r in cells; centre in cells at t0; travel axis, depth axis,
# sign, cells per step), runner, steps, fused, clamped axes, physical px range)
WIDE = {
    # a plate thinner than the depth support, centre on the top surface (high edge of axis 2)
    'plate_k_high': ((64, 40, 10), dict(a=3, b=4, c_f=3, c_r=6, centre=(32, 20, 9.5), travel_axis=1, depth_axis=2,
                                        sign=1, cells_per_step=1.0), 'func', 3, None, (2,), (1, 128)),
    # transverse support wider than axis 1, centre next to its low edge
    'narrow_j_low': ((64, 12, 40), dict(a=5, b=3, c_f=3, c_r=4, centre=(32, 1.0, 20), travel_axis=0, depth_axis=2,
                                        sign=-1, cells_per_step=1.0), 'step', 3, True, (1,), (1, 128)),
    # the same, centre next to the high edge, a captured graph
    'narrow_j_high': ((64, 12, 40), dict(a=5, b=3, c_f=3, c_r=4, centre=(32, 10.0, 20), travel_axis=0, depth_axis=2,
                                         sign=1, cells_per_step=1.0), 'run', 4, False, (1,), (1, 128)),
    # clamped along both axes, <8, 32> lines
    'both_200': ((200, 10, 12), dict(a=4, b=4, c_f=5, c_r=8, centre=(100, 5.5, 7.0), travel_axis=0, depth_axis=1,
                                     sign=-1, cells_per_step=2.0), 'func', 3, None, (1, 2), (129, 256)),
    # <16, 64> lines; the centre starts above the grid along axis 1 and moves in: the box start crosses 0 under replay
    'both_600_moving_in': ((600, 10, 12), dict(a=40, b=4, c_f=3, c_r=3, centre=(300, 14.0, 6.0), travel_axis=1,
                                               depth_axis=2, sign=-1, cells_per_step=1.5), 'run', 6, True, (1, 2),
                           (513, 1024)),
    # centre below the grid along axis 1 moving in, on a thin plate: clamped along both
    'plate_moving_in_low': ((64, 40, 10), dict(a=3, b=4, c_f=12, c_r=12, centre=(32, -6.0, 9.0), travel_axis=1,
                                               depth_axis=2, sign=1, cells_per_step=2.0), 'run', 5, None, (1, 2),
                            (1, 128)),
    # lines of more than 1024 rows (workspace kernel), travel along axis 2 from its low edge, depth along axis 1
    'long_1040': ((1040, 8, 10), dict(a=100, b=3, c_f=3, c_r=5, centre=(520, 4.0, 1.0), travel_axis=2, depth_axis=1,
                                      sign=1, cells_per_step=1.0), 'step', 3, False, (1, 2), (1025, 1 << 30)),
}


@pytest.mark.parametrize('name', list(WIDE))
def test_support_wider_than_the_grid(mods, name):
    hip, orc = mods
    shape, sk, runner, nsteps, fused, clamped, px_range = WIDE[name]
    t0 = 0.75 * DT
    src = goldak(hip, t0=t0, **sk)
    g = check_vs_oracle(hip, orc, shape, src, runner, nsteps, t0=t0, fused=fused, label=name)
    assert px_range[0] <= g.layout.px <= px_range[1], g.layout.px
    assert tuple(a for a in (1, 2) if box_clamped(src, g, a)) == clamped
    check_energy(hip, orc, shape, src, runner, nsteps, t0=t0, fused=fused, label=name)


# Every (travel_axis, depth_axis) pair and both travel directions; the centre crosses the middle of the box at 1.25 cells
# per step over 4 steps.  Travel along axis 0 puts the front / rear split inside the solved lines.
ORIENT = [(ta, da) for ta in range(3) for da in range(3) if ta != da]


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('ta,da', ORIENT, ids=['t%d_d%d' % o for o in ORIENT])
def test_orientation_matrix(mods, ta, da, sign, fused):
    hip, orc = mods
    shape = (40, 36, 32)
    centre = [20.0, 17.0, 15.0]
    centre[ta] -= sign * 2.5
    src = goldak(hip, a=3, b=2.5, c_f=3, c_r=5, centre=centre, travel_axis=ta, depth_axis=da, sign=sign,
                 cells_per_step=1.25)
    check_vs_oracle(hip, orc, shape, src, 'step', 4, fused=fused, label='t%d_d%d_s%+d_%s' % (ta, da, sign, fused))


# Every way the correction assembles A0 (lines0_row); the support spans the whole of axis 0, so the x- and x+ faces and the
# holes carry source on exposed rows.
A0_FORMS = ['face_consts', 'robin_field_x', 'stale_packs', 'hand_built', 'no_boundary']


def _oracle_packs_step(orc, T, go, mato, prmo, packs_o, q, Tinf=300.0):
    p0 = packs_o[0]
    folded = orc.AxisCoeffPack(p0.coeff, p0.dir_mask, p0.dir_val, p0.qflux + q / (RHO * CP))
    return orc.adi_step_numba_coeff(T, go, mato, prmo, (folded, packs_o[1], packs_o[2]), Tinf=Tinf)


@pytest.mark.parametrize('theta', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('form', A0_FORMS)
def test_a0_assembly_forms(mods, form, theta):
    hip, orc = mods
    shape = (24, 30, 28)
    rng = np.random.default_rng(7)
    mask, kw, T0 = make_case(shape, DX, seed=3)
    g, go = hip.Grid3D(*shape, DX, mask), orc.Grid3D(*shape, DX, mask)
    mat, mato = hip.Material(RHO, CP, K), orc.Material(RHO, CP, K)
    prm, prmo = hip.Params(DT, theta), orc.Params(DT, theta)
    if form == 'robin_field_x':
        kw['robin_h'] = dict(kw['robin_h'], **{'x-': 500.0 + 4000.0 * rng.random(shape)})
    if form == 'no_boundary':
        kw = {}
    if form == 'hand_built':
        dm = kw['dir_mask']
        arrs = [(2e3 * rng.random(shape), 5e3 * rng.random(shape)) for _ in range(3)]
        packs = tuple(hip.AxisCoeffPack(c, dm, kw['dir_value'], q) for c, q in arrs)
        packs_o = tuple(orc.AxisCoeffPack(c, dm, kw['dir_value'], q) for c, q in arrs)
    else:
        packs = hip.precompute_coeff_packs_unified(g, mat, **kw)
        packs_o = orc.precompute_coeff_packs_unified(go, mato, **kw)
    if form == 'stale_packs':
        new = mask.copy()
        new[rng.random(shape) > 0.95] = False
        new[:, :, shape[2] // 2] = True
        g.mask = new
        go.mask = new
    sp = hip._sparse_arg(g, packs[0], False) & 1
    fc = hip._fc_arg(g, packs[0], sp)
    assert (sp, fc is not None) == {'face_consts': (1, True), 'robin_field_x': (1, False), 'stale_packs': (0, False),
                                    'hand_built': (0, False), 'no_boundary': (1, True)}[form]
    # travel along axis 0: the front / rear split and the support's ends fall inside the lines
    src = goldak(hip, a=3, b=3, c_f=6, c_r=8, centre=(11.0, 15.0, 14.0), travel_axis=0, depth_axis=2, sign=1,
                 cells_per_step=1.0)
    t = 2 * DT
    got = np.asarray(hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=src, t=t))
    want = _oracle_packs_step(orc, T0, go, mato, prmo, packs_o, src.sample(go, t + 0.5 * DT))
    err = rel_linf(got, want)
    print('A0 %s theta=%.1f vs oracle: rel_linf %.3e' % (form, theta, err))
    assert err <= 1e-12, err
    plain = orc.adi_step_numba_coeff(T0, go, mato, prmo, packs_o, Tinf=300.0)
    assert np.abs(want - plain).max() > 1.0
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])
    if form != 'no_boundary':
        dm = kw['dir_mask'] & go.mask
        np.testing.assert_array_equal(got[dm], kw['dir_value'][dm])
    # the field form of the same step is the same step
    field = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=src.sample(go, t + 0.5 * DT))
    assert rel_linf(got, field) <= 1e-12


# Padded layouts and line lengths at the form switches: (shape, physical extents, source, clamped axes)
PADDED = {
    # every axis padded; the support reaches past the logical box into the padding of axes 1 and 2
    'pad_100x70x70': ((100, 70, 70), (104, 72, 80), dict(a=3, b=3, c_f=3, c_r=5, centre=(88, 66.0, 65.0),
                                                         travel_axis=1, depth_axis=2, sign=1, cells_per_step=1.0)),
    # physical px = 1024, the longest line solved in registers (<16, 64>)
    'px_1024': ((1009, 12, 40), (1024, 12, 48), dict(a=4, b=3, c_f=6, c_r=6, centre=(1000, 6.0, 37.0), travel_axis=0,
                                                     depth_axis=2, sign=1, cells_per_step=1.0)),
    # px = 1025, the shortest line of the workspace kernel
    'px_1025': ((1025, 12, 40), (1025, 12, 48), dict(a=4, b=3, c_f=6, c_r=6, centre=(10, 6.0, 37.0), travel_axis=0,
                                                     depth_axis=2, sign=-1, cells_per_step=1.0)),
    # a ragged logical nx padded to the first <8, 32> extent
    'px_144': ((129, 12, 40), (144, 12, 48), dict(a=3, b=3, c_f=4, c_r=4, centre=(126, 3.0, 30.0), travel_axis=1,
                                                  depth_axis=2, sign=-1, cells_per_step=1.0)),
    # a ragged physical px one row past the <8, 32> / <16, 32> switch
    'px_257': ((257, 10, 12), (257, 10, 12), dict(a=3, b=3, c_f=4, c_r=4, centre=(250, 5.0, 8.0), travel_axis=2,
                                                  depth_axis=1, sign=1, cells_per_step=1.0)),
}


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('name', list(PADDED))
def test_padding_and_line_lengths(mods, name, fused):
    hip, orc = mods
    shape, phys, sk = PADDED[name]
    src = goldak(hip, **sk)
    g = check_vs_oracle(hip, orc, shape, src, 'step', 3, fused=fused, label='%s_%s' % (name, fused))
    assert (g.layout.px, g.layout.py, g.layout.pz) == phys
    assert g.layout.padded == (phys != shape)
    # the padding comes back untouched: zero, as the layout allocated it
    mask, kw, T0 = make_case(shape, DX)
    mat = hip.Material(RHO, CP, K)
    packs = hip.precompute_coeff_packs_unified(g, mat, **kw)
    st = hip.StagedStepper(g, mat, hip.Params(DT, 0.5), packs, Tinf=300.0, fused=fused, source=src)
    T = st.step(hip.to_device(T0), t=0.0)
    px, py, pz, sx = g.layout.pd
    full = T.t.as_strided((px, py, pz), (sx, pz, 1)).cpu().numpy()
    inside = np.zeros((px, py, pz), bool)
    inside[:shape[0], :shape[1], :shape[2]] = True
    assert np.all(full[~inside] == 0.0)


# The single-track driver on a plate four cells thick under a source whose depth support is about 29 cells: the launch
# box is clamped along axis 2 (and along axis 1, the travel axis).
PLATE = dict(shape=(16, 20, 8), dx=2.5e-4, plate_k=4, box=(6, 10, 4, 6, 6))


def _plate_source(hip):
    return hip.GoldakSource(600.0, 0.7, 5e-4, 1e-3, 5e-4, 1e-3)


def test_thin_plate_driver_vs_oracle(mods):
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    (nx, ny, nz), dx, box = PLATE['shape'], PLATE['dx'], PLATE['box']
    plate = np.zeros((nx, ny, nz), dtype=bool)
    plate[:, :, :PLATE['plate_k']] = True
    h, Tinf, T_track, theta, dt, t_step = 20.0, 300.0, 1800.0, 0.5, 0.02, 0.05
    src = _plate_source(hip)
    assert 2 * R_CUT * src.b / dx > nz + 4
    got = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), h, Tinf, T_track, theta, dt, t_step,
                                heat_source=src)
    x0, x1, z0, z1, ncol = box
    mask = plate.copy()
    T = np.full((nx, ny, nz), Tinf)
    mat = orc.Material(RHO, CP, K)
    robin = {f: h for f in FACES}
    for yi in range(ncol):
        mask[x0:x1, yi:yi + 1, z0:z1] = True
        grid = orc.Grid3D(nx, ny, nz, dx, mask)
        T[x0:x1, yi:yi + 1, z0:z1] = T_track
        n_sub = max(1, int(np.ceil(t_step / dt)))
        prm = orc.Params(t_step / n_sub, theta)
        s = waam.track_source(src, box, dx, yi, t_step)
        for i in range(n_sub):
            q = s.sample(grid, i * prm.dt + 0.5 * prm.dt)
            T = oracle_step(orc, T, grid, mat, prm, dict(robin_h=robin, robin_Tinf=Tinf), q, Tinf=Tinf)
    err = rel_linf(got, T)
    print('thin plate driver vs oracle: rel_linf %.3e' % err)
    assert err <= 1e-10, err


def test_thin_plate_driver_energy(mods):
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    (nx, ny, nz), dx, box = PLATE['shape'], PLATE['dx'], PLATE['box']
    plate = np.zeros((nx, ny, nz), dtype=bool)
    plate[:, :, :PLATE['plate_k']] = True
    theta, dt, t_step = 0.5, 0.02, 0.05
    src = _plate_source(hip)
    got = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), 0.0, 0.0, 0.0, theta, dt, t_step,
                                heat_source=src)
    x0, x1, z0, z1, ncol = box
    mask = plate.copy()
    e_in = 0.0
    for yi in range(ncol):
        mask[x0:x1, yi:yi + 1, z0:z1] = True
        grid = orc.Grid3D(nx, ny, nz, dx, mask)
        n_sub = max(1, int(np.ceil(t_step / dt)))
        sdt = t_step / n_sub
        s = waam.track_source(src, box, dx, yi, t_step)
        e_in += sum(sdt * dx ** 3 * s.sample(grid, i * sdt + 0.5 * sdt).sum() for i in range(n_sub))
    e_field = RHO * CP * dx ** 3 * np.asarray(got)[mask].sum()
    print('thin plate driver energy: field / input - 1 = %.3e' % (e_field / e_in - 1.0))
    assert e_in > 0
    assert abs(e_field - e_in) <= 1e-11 * e_in, (e_field, e_in)
