"""GPU: the moving Goldak source of the Cartesian step (S= of adi_step_numba_coeff, source= of StagedStepper, heat_source= of
waam.run_single_track) against the pinned CPU oracle with the source folded into the axis-0 pack's qflux -- the oracle's
axis-0 right-hand side is out + dt*qflux + dt*coeff*Tinf, so qflux + q/(rho cp) is exactly the definition
R0 += dt*q(t + dt/2)/(rho cp) on in-mask, non-Dirichlet rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

RHO, CP, K = 7800.0, 500.0, 30.0
KAPPA = K / (RHO * CP)
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


def make_case(shape, dx=1e-4, holes=True, dirichlet=True, robin=True, neumann=True, seed=0):
    rng = np.random.default_rng(seed)
    mask = np.ones(shape, dtype=bool)
    if holes:
        mask &= rng.random(shape) > 0.08
        mask[:, :, -2:] = False                                 # a free surface on top
        mask[shape[0] // 2 - 1:shape[0] // 2 + 2, shape[1] // 2:shape[1] // 2 + 3, :] = False   # a hole under the path
    dm = (rng.random(shape) < 0.02) & mask if dirichlet else None
    dv = 300.0 + 20.0 * rng.random(shape) if dirichlet else None
    kw = dict(dir_mask=dm, dir_value=dv, robin_h={f: 25.0 + i for i, f in enumerate(FACES)} if robin else None,
              neumann={'z-': 2e4, 'x+': -5e3} if neumann else None)
    T0 = 300.0 + 40.0 * rng.random(shape)
    return mask, kw, T0


def source(hip, shape, dx, velocity=0.0, **kw):
    d = dict(power=800.0, eta=0.8, a=3e-4, b=2.5e-4, c_f=3e-4, c_r=6e-4, f_f=0.6,
             origin=(0.5 * shape[0] * dx, 0.3 * shape[1] * dx, (shape[2] - 2) * dx), velocity=velocity, travel_axis=1,
             travel_sign=1, depth_axis=2)
    d.update(kw)
    return hip.GoldakSource(**d)


def oracle_step(orc, T, grid, mat, prm, kw, q, Tinf=300.0):
    packs = orc.precompute_coeff_packs_unified(grid, mat, **kw)
    packs[0].qflux = packs[0].qflux + q / (RHO * CP)
    return orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)


def setup(hip, orc, shape, dx, dt, **case):
    mask, kw, T0 = make_case(shape, dx, **case)
    g = hip.Grid3D(*shape, dx, mask)
    go = orc.Grid3D(*shape, dx, mask)
    mat, mato = hip.Material(RHO, CP, K), orc.Material(RHO, CP, K)
    prm, prmo = hip.Params(dt, 0.5), orc.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, **kw)
    return g, go, mat, mato, prm, prmo, packs, kw, T0


CASES = [dict(shape=(37, 29, 45), holes=True, dirichlet=True, robin=True, neumann=True),
         dict(shape=(64, 64, 64), holes=False, dirichlet=False, robin=True, neumann=False)]


@pytest.mark.parametrize('case', CASES, ids=['mixed_37x29x45', 'solid_64'])
def test_field_form_vs_oracle(mods, case):
    hip, orc = mods
    c = dict(case)
    shape = c.pop('shape')
    dx, dt = 1e-4, 0.8 * 1e-8 / KAPPA
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, dx, dt, **c)
    src = source(hip, shape, dx)
    q = src.sample(go, 0.5 * dt)
    assert q.max() > 0
    got = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=q)
    want = oracle_step(orc, T0, go, mato, prmo, kw, q)
    assert rel_linf(got, want) <= 1e-12
    assert rel_linf(want, orc.adi_step_numba_coeff(T0, go, mato, prmo, orc.precompute_coeff_packs_unified(go, mato, **kw),
                                                  Tinf=300.0)) > 1e-4          # the source matters at this scale
    # the device sampler is the host one
    assert rel_linf(np.asarray(src.sample_device(g, 0.5 * dt)), q) <= 1e-14


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('case', CASES, ids=['mixed_37x29x45', 'solid_64'])
def test_analytic_source_vs_oracle_and_field(mods, case, fused):
    hip, orc = mods
    c = dict(case)
    shape = c.pop('shape')
    dx, dt = 1e-4, 0.8 * 1e-8 / KAPPA
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, dx, dt, **c)
    src = source(hip, shape, dx, velocity=0.05)
    t = 3 * dt
    st = hip.StagedStepper(g, mat, prm, packs, Tinf=300.0, fused=fused, source=src)
    got = np.asarray(st.step(hip.to_device(T0), t=t))
    q = src.sample(go, t + 0.5 * dt)
    assert rel_linf(got, oracle_step(orc, T0, go, mato, prmo, kw, q)) <= 1e-12
    field = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=q)
    assert rel_linf(got, field) <= 1e-12
    func = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=src, t=t)
    assert rel_linf(func, field) <= 1e-12


# one grid per line form of the correction kernel: k_source_lines0<8, 32> (physical nx 129 - 256), <16, 32> (257 - 512),
# <16, 64> (513 - 1024) and the workspace kernel for lines longer than 1024 rows; the source's support lies inside the box
LONG_LINES = [((200, 12, 16), (129, 256)), ((300, 12, 16), (257, 512)), ((600, 10, 16), (513, 1024)),
              ((1040, 8, 16), (1025, 1 << 30))]


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('shape,px_range', LONG_LINES, ids=['x'.join(map(str, c[0])) for c in LONG_LINES])
def test_line_forms_vs_oracle(mods, shape, px_range, fused):
    hip, orc = mods
    dx = 1e-4
    dt = 0.5 * dx * dx / KAPPA
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, dx, dt, holes=True, dirichlet=True, robin=True,
                                                       neumann=True)
    assert px_range[0] <= g.layout.px <= px_range[1], g.layout.px
    L = 1.2e-4                                            # support +-4.4 cells: inside the 8 - 16 cells of axes 1 and 2
    src = hip.GoldakSource(900.0, 0.8, L, L, L, 1.5 * L, f_f=0.7, origin=(0.55 * shape[0] * dx, 0.5 * shape[1] * dx,
                                                                         0.5 * shape[2] * dx), velocity=0.01)
    st = hip.StagedStepper(g, mat, prm, packs, Tinf=300.0, fused=fused, source=src)
    T = hip.to_device(T0)
    To = T0.copy()
    for n in range(3):
        T = st.step(T, t=n * dt)
        To = oracle_step(orc, To, go, mato, prmo, kw, src.sample(go, n * dt + 0.5 * dt))
    got = np.asarray(T)
    assert rel_linf(got, To) <= 1e-10                     # the issue's bar for several steps of a moving source
    plain = orc.adi_run(T0, go, mato, prmo, orc.precompute_coeff_packs_unified(go, mato, **kw), Tinf=300.0, nsteps=3)
    assert np.abs(got - plain).max() > 1.0               # the source reached the field
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])


def test_moving_source_20_steps_vs_oracle(mods):
    hip, orc = mods
    shape, dx = (40, 48, 24), 1e-4
    dt = 0.5 * dx * dx / KAPPA
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, dx, dt, holes=True, dirichlet=False, robin=True,
                                                       neumann=False)
    # travels along +axis 1 across the hole and off the far end of the surface
    src = source(hip, shape, dx, velocity=0.6 * shape[1] * dx / (20 * dt), origin=(20 * dx, 8 * dx, 22 * dx))
    T = hip.to_device(T0)
    To = T0.copy()
    for n in range(20):
        T = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=300.0, S=src, t=n * dt)
        To = oracle_step(orc, To, go, mato, prmo, kw, src.sample(go, n * dt + 0.5 * dt))
    assert rel_linf(np.asarray(T), To) <= 1e-10
    assert np.asarray(T).max() > T0.max() + 5.0


@pytest.mark.parametrize('fused', [True, False])
def test_graph_replay_is_the_step_loop(mods, fused):
    hip, orc = mods
    shape, dx = (40, 48, 32), 1e-4
    dt = 0.5 * dx * dx / KAPPA
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, dx, dt, holes=True, dirichlet=True, robin=True,
                                                       neumann=True)
    src = source(hip, shape, dx, velocity=0.2, origin=(20 * dx, 10 * dx, 30 * dx))
    st = hip.StagedStepper(g, mat, prm, packs, Tinf=300.0, fused=fused, source=src)
    T = hip.to_device(T0)
    t0 = 0.37 * dt

    def loop(n):
        X = T
        for i in range(n):
            X = st.step(X, t=t0 + i * dt)
        return np.asarray(X)
    for n in (6, 7):
        np.testing.assert_array_equal(np.asarray(st.run(T, n, t0=t0)), loop(n))
    caps = st.captures
    src.power = 1300.0
    src.origin = (18 * dx, 14 * dx, 30 * dx)
    src.velocity = 0.35
    np.testing.assert_array_equal(np.asarray(st.run(T, 6, t0=t0)), loop(6))
    assert st.captures == caps                     # the block moved, the graph stayed
    src.a = 4e-4                                   # a new support extent: a new graph
    np.testing.assert_array_equal(np.asarray(st.run(T, 6, t0=t0)), loop(6))
    assert st.captures == caps + 1


def test_energy_balance_adiabatic(mods):
    hip, orc = mods
    shape, dx = (36, 44, 28), 1e-4
    dt = 0.5 * dx * dx / KAPPA
    mask, _, _ = make_case(shape, dx, holes=True)
    g = hip.Grid3D(*shape, dx, mask)
    go = orc.Grid3D(*shape, dx, mask)
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat)
    src = source(hip, shape, dx, velocity=0.5 * shape[1] * dx / (50 * dt), origin=(18 * dx, 10 * dx, 25 * dx))
    T = hip.to_device(np.zeros(shape))
    st = hip.StagedStepper(g, mat, prm, packs, source=src)
    TN = np.asarray(st.run(T, 50, t0=0.0))
    e_field = RHO * CP * dx ** 3 * TN[mask].sum()
    e_in = sum(dt * src.sample(go, n * dt + 0.5 * dt).sum() * dx ** 3 for n in range(50))
    assert e_in > 0
    assert abs(e_field - e_in) <= 1e-11 * e_in, (e_field, e_in)


def test_mask_and_identity_behaviour(mods):
    hip, orc = mods
    shape, dx = (37, 29, 45), 1e-4
    dt = 0.5 * dx * dx / KAPPA
    g, go, mat, mato, prm, prmo, packs, kw, T0 = setup(hip, orc, shape, dx, dt)
    src = source(hip, shape, dx, velocity=0.1)
    plain = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0)
    got = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=src, t=2 * dt)
    mask = go.mask
    np.testing.assert_array_equal(got[~mask], T0[~mask])
    dm = kw['dir_mask']
    np.testing.assert_array_equal(got[dm], kw['dir_value'][dm])
    assert np.abs(got - plain).max() > 1.0
    np.testing.assert_array_equal(hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=None), plain)
    np.testing.assert_array_equal(hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=np.zeros(shape)), plain)
    # a support that misses the mask: beyond the box and above the free surface
    far = source(hip, shape, dx, origin=(0.5 * shape[0] * dx, 0.5 * shape[1] * dx, (shape[2] + 10) * dx))
    assert far.sample(go, 0.0).max() == 0.0
    np.testing.assert_array_equal(hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=far), plain)
    st = hip.StagedStepper(g, mat, prm, packs, Tinf=300.0, source=far)
    np.testing.assert_array_equal(np.asarray(st.run(hip.to_device(T0), 4)),
                                  np.asarray(hip.StagedStepper(g, mat, prm, packs, Tinf=300.0).run(hip.to_device(T0), 4)))


# The bar of the physics check is the oracle's own discretisation error on this very configuration (computed below on
# the CPU, 3.4e-3 at dt = dx^2 / (2 kappa) and 40 steps after the source step) with a margin of 2x; the oracle's error
# itself must stay below PHYSICS_ORACLE_MAX, so a broken oracle cannot widen the bar.
PHYSICS_MARGIN = 2.0
PHYSICS_ORACLE_MAX = 5e-3


def test_stationary_source_relaxes_to_the_diffusing_gaussian(mods):
    hip, orc = mods
    n, dx, L, P, eta, N = 64, 1e-4, 6e-4, 200.0, 1.0, 40
    dt = 0.5 * dx * dx / KAPPA
    g = hip.Grid3D(n, n, n, dx, np.ones((n, n, n), dtype=bool))
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat)
    src = hip.GoldakSource(P, eta, L, L, L, L, f_f=1.0, origin=(32 * dx, 32 * dx, 32 * dx))
    T = hip.adi_step_numba_coeff(hip.to_device(np.zeros((n, n, n))), g, mat, prm, packs, S=src, t=0.0)
    T = np.asarray(hip.StagedStepper(g, mat, prm, packs).run(T, N))
    # the oracle on the same configuration: source step (qflux fold), then N plain steps
    go, mato, prmo = orc.Grid3D(n, n, n, dx, np.ones((n, n, n), dtype=bool)), orc.Material(RHO, CP, K), orc.Params(dt, 0.5)
    To = oracle_step(orc, np.zeros((n, n, n)), go, mato, prmo, {}, src.sample(go, 0.5 * dt), Tinf=0.0)
    To = orc.adi_run(To, go, mato, prmo, orc.precompute_coeff_packs_unified(go, mato), nsteps=N)
    assert rel_linf(T, To) <= 1e-10
    t = N * dt + 0.5 * dt
    s2 = L * L / 6.0
    sf2 = s2 + 2.0 * KAPPA * t
    x = (np.arange(n) + 0.5) * dx - 32 * dx
    q0 = 6.0 * np.sqrt(3.0) * eta * P / (L ** 3 * np.pi ** 1.5)
    g1 = np.exp(-x * x / (2.0 * sf2)) * np.sqrt(s2 / sf2)
    Ta = dt * q0 / (RHO * CP) * g1[:, None, None] * g1[None, :, None] * g1[None, None, :]
    err, err_oracle = rel_linf(T, Ta), rel_linf(To, Ta)
    assert err_oracle <= PHYSICS_ORACLE_MAX, err_oracle
    assert err <= PHYSICS_MARGIN * err_oracle, (err, err_oracle)


def test_single_track_driver_with_heat_source(mods):
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    nx, ny, nz, dx = 16, 20, 14, 2.5e-4
    plate = np.zeros((nx, ny, nz), dtype=bool)
    plate[:, :, :6] = True
    box = (6, 10, 6, 9, 6)
    h, Tinf, T_track, theta, dt, t_step = 20.0, 300.0, 1800.0, 0.5, 0.02, 0.05
    src = hip.GoldakSource(600.0, 0.7, 5e-4, 4e-4, 5e-4, 1e-3)
    got = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), h, Tinf, T_track, theta, dt, t_step, heat_source=src)
    # the same loop on the oracle: same births, the source folded into qflux
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
    assert rel_linf(got, T) <= 1e-10
    plain = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), h, Tinf, T_track, theta, dt, t_step)
    assert np.asarray(got).max() > np.asarray(plain).max() + 1.0
