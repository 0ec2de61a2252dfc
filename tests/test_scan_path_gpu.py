"""GPU: the scan path of the Goldak source as a source field of the step, adi_step_numba_coeff(..., S=path.sample_step(grid, t,
dt)), against the pinned CPU oracle with sample_step/(rho cp) folded into the axis-0 pack's qflux (the method of
test_heat_source_gpu.py, on the mask, Dirichlet, Robin and Neumann mix of its make_case, the hole under the path included)."""
import numpy as np
import pytest

import scan_cases as sc
from scan_cases import DT, DX, RHO, CP, K, rel_linf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


def _step(hip, T, g, mat, prm, packs, q):
    return hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=300.0, S=q)


# ------------------------------------------------------------------------------------------------- one step against the oracle
def _two_leg_path(hip, shape, s, t_start):
    """an oblique leg along the lines and a corner into +v, under the free surface, over the hole of make_case; 1.6 DT in all"""
    nx, ny, nz = shape
    z = (nz - 2) * DX
    p = hip.ScanPath(power=800.0, start=(0.5 * nx * DX - 7 * DX, 0.5 * ny * DX - 1.5 * DX, z), t_start=t_start, **s)
    v = (np.hypot(9.0, 2.0) + 2.5) * DX / (1.6 * DT)
    return p.line_to((0.5 * nx * DX + 2 * DX, 0.5 * ny * DX + 0.5 * DX, z), v).line_to((0.5 * nx * DX + 2 * DX, 0.5 * ny * DX + 3 * DX, z), v)


@pytest.mark.parametrize('shape,s', [((37, 29, 45), sc.SHAPE), ((130, 12, 20), sc.SMALL)], ids=['37x29x45', '130x12x20'])
def test_field_form_vs_oracle(mods, shape, s):
    """a step that holds a corner; the field is sampled on the device grid (a real Grid3D and its mask) and on the oracle's"""
    hip, orc = mods
    g, go, mat, mato, prm, prmo, packs, kw, T0 = sc.setup(hip, orc, shape)
    path = _two_leg_path(hip, shape, s, 0.25 * DT)
    t = 0.6 * DT                                            # the step [0.6, 1.6] DT holds the corner (at 1.51 DT)
    q = path.sample_step(g, t, DT)
    np.testing.assert_array_equal(q, path.sample_step(go, t, DT))
    assert q.max() > 0 and path._piece(0, t, t + DT) and path._piece(1, t, t + DT)
    np.testing.assert_array_equal(q[~go.mask], 0.0)
    got = _step(hip, T0, g, mat, prm, packs, q)
    want = sc.oracle_step(orc, T0, go, mato, prmo, kw, q)
    err = rel_linf(got, want)
    print('%s: field form vs oracle %.2e' % (shape, err))
    assert err <= 1e-12
    plain = orc.adi_step_numba_coeff(T0, go, mato, prmo, orc.precompute_coeff_packs_unified(go, mato, **kw), Tinf=300.0)
    assert rel_linf(want, plain) > 1e-4                     # the source matters at this scale
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])


# ----------------------------------------------------------------------------------------------------------------- windows
def _window_path(hip, shape):
    """t_start = 2 DT; leg A 3 DT, a jump 0.5 DT, leg B 2.5 DT, a dwell without power 3 DT, leg C 2 DT"""
    nx, ny, nz = shape
    z = (nz - 2) * DX
    x, y = 0.5 * nx * DX, 0.3 * ny * DX
    p = hip.ScanPath(power=800.0, start=(x, y, z), t_start=2 * DT, **sc.SHAPE)
    p.line_to((x, y + 6 * DX, z), 6 * DX / (3 * DT))
    p.line_to((x + 4 * DX, y + 6 * DX, z), 4 * DX / (0.5 * DT), power=0.0)
    p.line_to((x + 4 * DX, y + 1 * DX, z), 5 * DX / (2.5 * DT))
    p.dwell(3 * DT)
    p.line_to((x - 2 * DX, y + 1 * DX, z), 6 * DX / (2 * DT))
    return p


WINDOWS = [('inside_one_segment', 3.0, [0]), ('on_a_boundary', 'tab1', [1, 2]), ('three_segments_one_a_jump', 4.6, [0, 1, 2]),
           ('before_t_start', 0.5, None), ('after_t_end', 'end', None), ('inside_an_idle_dwell', 9.0, None)]


@pytest.mark.parametrize('name,when,segs', WINDOWS, ids=[w[0] for w in WINDOWS])
def test_windows(mods, name, when, segs):
    hip, orc = mods
    shape = (37, 29, 45)
    g, go, mat, mato, prm, prmo, packs, kw, T0 = sc.setup(hip, orc, shape)
    path = _window_path(hip, shape)
    t = {'tab1': path.table()[1, 0], 'end': path.t_end + 0.25 * DT}.get(when, None)
    t = when * DT if t is None else t
    overl = [k for k in range(path.n_segments) if min(t + DT, path._t_next(k)) > max(t, path.table()[k, 0])]
    q = path.sample_step(g, t, DT)
    got = _step(hip, T0, g, mat, prm, packs, q)
    if segs is None:
        assert not q.any()                                  # nothing deposits: the field form of the step without a source
        np.testing.assert_array_equal(got, _step(hip, T0, g, mat, prm, packs, np.zeros(shape)))
        assert rel_linf(got, hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0)) <= 1e-12
    else:
        assert overl == segs and q.max() > 0
        err = rel_linf(got, sc.oracle_step(orc, T0, go, mato, prmo, kw, q))
        print('%s: vs oracle %.2e' % (name, err))
        assert err <= 1e-12


# -------------------------------------------------------------------------------------------------------------- grid edges
def _edge_paths(hip, shape):
    nx, ny, nz = shape
    X = 0.3 * nx * DX
    leg = lambda s, y, z, ang=0.0, **k: sc.leg_path(hip, s, (X, y, z), ang, 8 * DX, 8 * DX / (0.8 * DT), t_start=0.1 * DT, **k)
    wide = dict(sc.SHAPE, a=2.5e-3, b=2.5e-3)              # 91 cells each side: wider than the grid along axes 1 and 2
    return {'axis1_low': leg(sc.SHAPE, 1.5 * DX, 0.5 * nz * DX), 'axis1_high': leg(sc.SHAPE, (ny - 1.5) * DX, 0.5 * nz * DX),
            'axis2_low': leg(sc.SHAPE, 0.5 * ny * DX, 1.5 * DX), 'axis2_high': leg(sc.SHAPE, 0.5 * ny * DX, (nz - 2) * DX),
            'both_sides': leg(wide, 0.5 * ny * DX, 0.5 * nz * DX),
            'oblique_over_the_corner': leg(sc.SHAPE, 2.5 * DX, 2.0 * DX, ang=-30.0),
            'centre_outside': leg(sc.SHAPE, -2.0 * DX, (nz + 1) * DX, ang=20.0)}


EDGES = ['axis1_low', 'axis1_high', 'axis2_low', 'axis2_high', 'both_sides', 'oblique_over_the_corner', 'centre_outside']


@pytest.mark.parametrize('name', EDGES)
def test_grid_edges(mods, name):
    """the support overhangs the low and the high side of axis 1 and of axis 2, and both at once"""
    hip, orc = mods
    shape = (33, 21, 19)
    g, go, mat, mato, prm, prmo, packs, kw, T0 = sc.setup(hip, orc, shape)
    path = _edge_paths(hip, shape)[name]
    q = path.sample_step(g, 0.0, DT)
    _, jj, kk = np.nonzero(q)
    assert q.max() > 0
    lo1, hi1, lo2, hi2 = jj.min() == 0, jj.max() == shape[1] - 1, kk.min() == 0, kk.max() >= shape[2] - 3   # (two planes off the mask)
    assert {'axis1_low': lo1, 'axis1_high': hi1, 'axis2_low': lo2, 'axis2_high': hi2, 'both_sides': lo1 and hi1 and lo2 and hi2,
            'oblique_over_the_corner': lo1 and lo2, 'centre_outside': lo1 and hi2}[name]
    err = rel_linf(_step(hip, T0, g, mat, prm, packs, q), sc.oracle_step(orc, T0, go, mato, prmo, kw, q))
    print('%s: vs oracle %.2e' % (name, err))
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------------------ twenty steps
def test_raster_20_steps_vs_oracle(mods):
    hip, orc = mods
    shape = (40, 48, 24)
    g, go, mat, mato, prm, prmo, packs, kw, T0 = sc.setup(hip, orc, shape)
    length = 3 * 20 * DX + 2 * 8 * DX
    path = hip.ScanPath.raster((10 * DX, 14 * DX), (30 * DX, 30.5 * DX), 8 * DX, length / (19.3 * DT), 800.0, depth=22 * DX,
                               t_start=0.4 * DT, **sc.SHAPE)
    assert path.n_segments == 5 and path.t_end < 20 * DT     # three tracks, two turns, all of it inside the run
    T, To = hip.to_device(T0), T0.copy()
    for n in range(20):
        q = path.sample_step(g, n * DT, DT)
        T = _step(hip, T, g, mat, prm, packs, q)
        To = sc.oracle_step(orc, To, go, mato, prmo, kw, q)
    got = np.asarray(T)
    err = rel_linf(got, To)
    print('raster, 20 steps: vs oracle %.2e' % err)
    assert err <= 1e-10                                     # the project's bar for several steps of a moving source
    assert got.max() > T0.max() + 5.0
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])
    dm = kw['dir_mask']
    assert dm.any()
    np.testing.assert_array_equal(got[dm], To[dm])
    np.testing.assert_array_equal(got[dm], kw['dir_value'][dm])


# -------------------------------------------------------------------------------------------------------- adiabatic energy
def test_adiabatic_energy(mods):
    """rho cp sum (T - T0) dx^3 against the sum over the steps of sum sample_step dx^3 dt on an all-solid adiabatic box"""
    hip, orc = mods
    shape = (48, 40, 24)
    g = hip.Grid3D(*shape, DX, np.ones(shape, dtype=bool))
    mat, prm = hip.Material(RHO, CP, K), hip.Params(DT, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat)
    path = sc.tour_path(hip, sc.SHAPE, (20 * DX, 12 * DX, 20 * DX), 10 * DX, 4.5 * 10 * DX / (11.4 * DT), t_start=0.3 * DT)
    n = 12
    assert path.t_end < n * DT
    T = hip.to_device(np.zeros(shape))
    e_in = 0.0
    for i in range(n):
        q = path.sample_step(g, i * DT, DT)
        e_in += DT * q.sum() * DX ** 3
        T = hip.adi_step_numba_coeff(T, g, mat, prm, packs, S=q)
    e_field = RHO * CP * DX ** 3 * np.asarray(T).sum()
    assert e_in > 0
    err = abs(e_field - e_in) / e_in
    print('adiabatic energy: %.2e' % err)
    assert err <= 1e-11


# ------------------------------------------------------------------------------------------------ a path is not a device source
def test_a_path_itself_is_refused(mods):
    """the step and the stepper say that a path comes in as its field instead of taking it for something else"""
    hip, orc = mods
    shape = (16, 12, 10)
    g = hip.Grid3D(*shape, DX, np.ones(shape, dtype=bool))
    mat, prm = hip.Material(RHO, CP, K), hip.Params(DT, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat)
    path = sc.leg_path(hip, sc.SMALL, (4 * DX, 5 * DX, 5 * DX), 0.0, 6 * DX, 0.4)
    with pytest.raises(TypeError, match='sample_step'):
        hip.adi_step_numba_coeff(np.zeros(shape), g, mat, prm, packs, S=path)
    with pytest.raises(TypeError, match='sample_step'):
        hip.StagedStepper(g, mat, prm, packs, source=path)
