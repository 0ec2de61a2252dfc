"""GPU: the temperature-dependent surface loss on the device -- adi_surface_loss_update through LossPacks, the `surface_loss=`
argument of adi_step_numba_coeff / StagedStepper and of the waam loops -- against the golden vectors of the reference
(tests/golden/make_golden_surface_loss.py) and, where the reference has no vectors, against the lagged loop over the pinned C
oracle that tests/test_surface_loss_cpu.py holds to those vectors.

Bars: coefficient arrays np.array_equal (IEEE add / multiply / divide in one fixed order on both sides, contraction off); fields
<= 1e-10 relative L-inf, the project's bar; graph replay against the same launches issued one by one: bit-identical."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import surface_loss_cases as slc  # noqa: E402
from surface_loss_cases import FACES, rel_linf  # noqa: E402

pytestmark = pytest.mark.gpu

RHO, CP, K = 7800.0, 490.0, 54.0
KAPPA = K / (RHO * CP)


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


# every golden case on the box the library picks for it ('long' is padded along axis 2), and 'holes' once more on a padded
# physical box whose rows are whole 16-byte pieces (the packed flag loads, cells of the box outside the logical grid)
VARIANTS = [('holes', None), ('holes', (12, 8, 16)), ('long', None), ('birth', None), ('table', None), ('plain', None)]
IDS = ['holes', 'holes_padded', 'long', 'birth', 'table', 'plain']


def _pad(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _coeffs(lp):
    return [p.coeff for p in lp.packs]


def _assert_coeffs(lp, c, key, what):
    for ax, got in zip('xyz', _coeffs(lp)):
        want = c[key % ax]
        assert got.shape == want.shape and np.array_equal(got, want), \
            (what, ax, int((got != want).sum()), float(np.abs(got - want).max()))


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_coeff_parity_construction_update_rebuild(mods, monkeypatch, name, phys):
    hip, _ = mods
    _pad(monkeypatch, hip, phys)
    c = slc.load(name)
    grid = hip.Grid3D(*c['mask'].shape, float(c['dx']), np.array(c['mask']))
    assert grid.layout.padded == (phys is not None or name == 'long')
    mat = hip.Material(RHO, CP, K)
    loss = slc.loss_of(c, hip.SurfaceLoss)
    Tinf = float(c['Tinf'])
    T = hip.to_device(np.array(c['T0']))
    lp = hip.LossPacks(grid, mat, loss, Tinf, T=T, **slc.bc_of(c))
    for p in lp.packs:
        assert p.sparse_ok and p.face_consts is None and p.mask_version == grid.mask_version
    ptrs = [p.d_coeff.data_ptr() for p in lp.packs]
    _assert_coeffs(lp, c, 'seg0_coeff_%s', 'construction')
    for ax, p in zip('xyz', lp.packs):
        assert np.array_equal(p.qflux, c['qflux_' + ax]), ax
    # update: the exposed cells follow the field, nothing else is written
    lp.update(hip.to_device(np.array(c['T0']) + 111.0))
    if name != 'plain':
        assert any(not np.array_equal(g, c['seg0_coeff_%s' % ax]) for ax, g in zip('xyz', _coeffs(lp)))
    lp.update(T)
    _assert_coeffs(lp, c, 'seg0_coeff_%s', 'update')
    for p in lp.packs:
        p.d_coeff.fill_(7.0)                         # update writes exposed cells only: the rest keeps the marker
    lp.update(T)
    for ax, got in zip('xyz', _coeffs(lp)):
        want = c['seg0_coeff_%s' % ax]
        a = 'xyz'.index(ax)
        m = np.pad(c['mask'], 1)
        sl = lambda d: tuple(slice(1 + (d if i == a else 0), 1 + (d if i == a else 0) + c['mask'].shape[i]) for i in range(3))
        exposed = c['mask'] & ~(m[sl(-1)] & m[sl(+1)])
        assert np.array_equal(got[exposed], want[exposed]) and np.all(got[~exposed] == 7.0), ax
    # rebuild: every cell, zeros where nothing is exposed
    lp.rebuild(T)
    _assert_coeffs(lp, c, 'seg0_coeff_%s', 'rebuild')
    assert ptrs == [p.d_coeff.data_ptr() for p in lp.packs]
    if name == 'plain':
        ref = hip.precompute_coeff_packs_unified(grid, mat, robin_h={f: float(v) for f, v in zip(FACES, c['h'])})
        for p, q in zip(lp.packs, ref):
            assert np.array_equal(p.coeff, q.coeff) and q.coeff.max() > 0


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_step_parity_with_the_reference(mods, monkeypatch, name, phys):
    """the whole golden sequence through adi_step_numba_coeff(surface_loss=): every T; the coefficient arrays after each birth
    (rebuild on the changed planes + the update a step starts with) at every cell, and those of the last step.  Bit equality
    of coefficients needs bit-equal temperatures, and the fields of the two sides differ in the last digits from the first
    step on: the arrays are compared for the REFERENCE's field at that point (the stored T, the birth applied), written to the
    same buffers by the same calls, after which the run goes on from the device's own field."""
    hip, _ = mods
    _pad(monkeypatch, hip, phys)
    import torch
    c = slc.load(name)
    shape = c['mask'].shape
    mask = np.array(c['mask'])
    grid = hip.Grid3D(*shape, float(c['dx']), mask)
    mat = hip.Material(RHO, CP, K)
    loss = slc.loss_of(c, hip.SurfaceLoss)
    Tinf = float(c['Tinf'])
    T = hip.to_device(np.array(c['T0']))
    births = 'full_mask' in c
    if births:                                            # the device loop of waam.run_layer_birth
        d_full = grid.layout.to_layout(np.array(c['full_mask']), torch.uint8)
        d_act = grid.layout.to_layout(mask, torch.uint8)
        grid.set_mask_device(d_act, all_solid=False)
    lp = hip.LossPacks(grid, mat, loss, Tinf, **slc.bc_of(c))
    worst = 0.0
    for s, dt, nsteps, k0, k1 in slc.segments(c):
        if k0 >= 0:
            nb = slc.born_mask(c, mask, k0, k1)
            mask |= nb
            hip.birth_planes(T, d_act, d_full, grid, k0, k1, float(c['Ts']))
            grid.set_mask_device(d_act, max(k0 - 1, 0), min(shape[2], k1 + 1), all_solid=False)
            Tg = np.array(c['seg%d_T%d' % (s - 1, int(c['seg%d_nsteps' % (s - 1)]))])
            Tg[nb] = float(c['Ts'])
            assert rel_linf(np.asarray(T), Tg) <= 1e-10
            Tg = hip.to_device(Tg)
            lp.rebuild(Tg, k0 - 1, k1 + 1)                # the planes whose exposure changed: stale cells zeroed
            lp.update(Tg)                                 # (what the next step does first)
            _assert_coeffs(lp, c, 'seg%d' % s + '_coeff_%s', 'birth %d' % s)
            assert np.array_equal(grid.mask, mask)
        prm = hip.Params(dt, float(c['theta']))
        for n in range(nsteps):
            prev = np.asarray(T)
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, lp.packs, Tinf=Tinf, surface_loss=lp)
            got = np.asarray(T)
            e = rel_linf(got, c['seg%d_T%d' % (s, n + 1)])
            worst = max(worst, e)
            print(name, 'segment', s, 'step', n + 1, 'rel L-inf %.3e' % e)
            assert e <= 1e-10, (name, s, n + 1, e)
            assert np.array_equal(got[~mask], prev[~mask])            # off-mask cells: bit-untouched
    lp.update(hip.to_device(np.array(c['seg%d_T%d' % (s, nsteps - 1)])))       # the field the reference's last step started from
    _assert_coeffs(lp, c, 'coeff_last_%s', 'last step')
    print(name, 'worst rel L-inf %.3e' % worst, 'promise ledger:', [sorted(map(str, set(p.__dict__.get('_nofb', {}).values())))
                                                                    for p in lp.packs])


# ---- graph replay on a 64 x 48 x 80 ellipsoid ----------------------------------------------------------------------------
SHAPE, DX = (64, 48, 80), 5e-4
DT, THETA, TINF = 2.0 * DX * DX / KAPPA, 0.5, 25.0


def _ellipsoid():
    x, y, z = [(np.arange(n) + 0.5) / n - 0.5 for n in SHAPE]
    X, Y, Z = np.meshgrid(x, y, z, indexing='ij')
    mask = (X / 0.46) ** 2 + (Y / 0.44) ** 2 + (Z / 0.48) ** 2 <= 1.0
    T0 = 760.0 + 700.0 * np.sin(5.0 * X + 0.3) * np.cos(4.0 * Y) * np.cos(6.0 * Z - 0.2)
    return mask, np.clip(T0, 20.0, 1500.0)


def _source(hip):
    return hip.GoldakSource(power=800.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                            origin=(32 * DX, 14 * DX, 60 * DX), velocity=0.02, travel_axis=1, travel_sign=1, depth_axis=2)


@pytest.fixture(scope='module')
def ell(mods):
    """the grid, and the oracle's lagged loop from T0 for 6 steps, without and with the moving source (computed once)"""
    hip, orc = mods
    mask, T0 = _ellipsoid()
    go, mato, prmo = orc.Grid3D(*SHAPE, DX, mask), orc.Material(RHO, CP, K), orc.Params(DT, THETA)
    loss = hip.SurfaceLoss(h=15.0, emissivity=0.8)
    src = _source(hip)
    seq = {False: [T0], True: [T0]}
    for with_src in (False, True):
        T = T0
        for i in range(6):
            packs = orc.precompute_coeff_packs_unified(go, mato, robin_h=slc.h_fields(loss, T, TINF))
            if with_src:
                packs[0].qflux = packs[0].qflux + src.sample(go, i * DT + 0.5 * DT) / (RHO * CP)
            T = orc.adi_step_numba_coeff(T, go, mato, prmo, packs, Tinf=TINF)
            seq[with_src].append(T)
    for v in seq.values():
        for a in v:
            a.setflags(write=False)
    assert rel_linf(seq[True][6], seq[False][6]) > 1e-4          # the source matters at this scale
    return dict(mask=mask, T0=T0, seq=seq)


def _explicit(hip, lp, plain, T, n, with_src):
    """n times: the update from the step's input, then the step without surface_loss -- the launches a graph of the stepper
    with surface_loss= replays, issued one by one"""
    cur = hip.to_device(T)
    for i in range(n):
        lp.update(cur)
        cur = plain.step(cur, t=i * DT) if with_src else plain.step(cur)
    return np.asarray(cur)


@pytest.mark.parametrize('with_src', [False, True], ids=['loss', 'loss+source'])
def test_graph_replay_recapture_and_law_change(mods, ell, with_src):
    hip, _ = mods
    grid = hip.Grid3D(*SHAPE, DX, ell['mask'])
    mat, prm = hip.Material(RHO, CP, K), hip.Params(DT, THETA)
    loss = hip.SurfaceLoss(h=15.0, emissivity=0.8)
    lp = hip.LossPacks(grid, mat, loss, TINF)
    src = _source(hip) if with_src else None
    st = hip.StagedStepper(grid, mat, prm, lp.packs, TINF, surface_loss=lp, source=src)
    plain = hip.StagedStepper(grid, mat, prm, lp.packs, TINF, source=src)
    T0 = ell['T0']
    for n in (5, 6):
        got = np.asarray(st.run(hip.to_device(T0), n, t0=0.0))
        e = rel_linf(got, ell['seq'][with_src][n])
        print('n =', n, 'graph vs oracle rel L-inf %.3e' % e)
        assert e <= 1e-10, (n, e)
        assert np.array_equal(got, _explicit(hip, lp, plain, T0, n, with_src)), n
        assert np.array_equal(got[~ell['mask']], T0[~ell['mask']])
    assert st.captures == 1
    # another field: the same graph
    T1 = np.where(ell['mask'], 0.5 * T0 + 300.0, T0)
    got = np.asarray(st.run(hip.to_device(T1), 6, t0=0.0))
    assert st.captures == 1
    assert np.array_equal(got, _explicit(hip, lp, plain, T1, 6, with_src))
    assert rel_linf(got, ell['seq'][with_src][6]) > 1e-3
    # another law: the launch holds it by value, so the graph is captured anew -- and the result is the ungraphed one
    loss.emissivity = 0.3
    got = np.asarray(st.run(hip.to_device(T0), 6, t0=0.0))
    assert st.captures == 2
    assert np.array_equal(got, np.asarray(st.run(hip.to_device(T0), 6, graph=False, t0=0.0)))
    assert np.array_equal(got, _explicit(hip, lp, plain, T0, 6, with_src))
    assert rel_linf(got, ell['seq'][with_src][6]) > 1e-4          # the emissivity matters
    # and the step() of the stepper runs the update itself
    one = np.asarray(st.step(hip.to_device(T0), t=0.0))
    assert np.array_equal(one, _explicit(hip, lp, plain, T0, 1, with_src))


def test_stepper_and_step_refuse_foreign_packs(mods, ell):
    hip, _ = mods
    grid = hip.Grid3D(*SHAPE, DX, ell['mask'])
    mat, prm = hip.Material(RHO, CP, K), hip.Params(DT, THETA)
    lp = hip.LossPacks(grid, mat, hip.SurfaceLoss(h=15.0), TINF)
    other = hip.precompute_coeff_packs_unified(grid, mat, robin_h=15.0)
    with pytest.raises(ValueError, match='own packs'):
        hip.StagedStepper(grid, mat, prm, other, TINF, surface_loss=lp)
    with pytest.raises(ValueError, match='own packs'):
        hip.adi_step_numba_coeff(hip.to_device(ell['T0']), grid, mat, prm, other, Tinf=TINF, surface_loss=lp)
    with pytest.raises(ValueError, match='Tinf'):
        hip.LossPacks(grid, mat, hip.SurfaceLoss(emissivity=0.5), -300.0)


# ---- the layer-birth loop ------------------------------------------------------------------------------------------------
def test_run_layer_birth_with_surface_loss(mods):
    """waam.run_layer_birth on a 12 x 10 x 14 head, cfl chosen so that the last segment takes the graph path and the others
    the step-by-step one, against the same event loop written here over the oracle"""
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    shape, dx = (12, 10, 14), 1e-3
    full = waam.synthetic_head_mask(*shape)
    layers = waam.plan_layers(full, 2)
    tb = waam.birth_times(full, layers, dx, bead_width=4e-3, scan_speed=8e-3)
    t_out = [tb[-1] + 6.0 * (tb[-1] - tb[-2])]
    Tinf, Ts, theta, cfl = 25.0, 1450.0, 0.5, 2.0
    loss = hip.SurfaceLoss(h=12.0, emissivity=0.85, table=([25.0, 500.0, 1500.0], [0.0, 6.0, 9.0]))
    dt_cap = cfl * dx * dx / KAPPA
    nsubs = [max(1, int(math.ceil(a / dt_cap))) for w, a in waam.layer_birth_schedule(tb, t_out) if w == 'advance']
    assert max(nsubs) >= waam.GRAPH_MIN_NSUB and min(nsubs) < waam.GRAPH_MIN_NSUB, nsubs
    got, nsteps = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), 0.0, Tinf, Ts, theta, cfl, layers, tb, t_out,
                                       surface_loss=loss)
    # the same loop over the oracle
    mask = np.zeros(shape, dtype=bool)
    grid, mat = orc.Grid3D(*shape, dx, mask), orc.Material(RHO, CP, K)
    T = np.full(shape, Tinf)
    want_steps = 0
    for what, arg in waam.layer_birth_schedule(tb, t_out):
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = orc.Params(max(arg / nsub, 1e-15), theta)
            for _ in range(nsub):
                packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=slc.h_fields(loss, T, Tinf))
                T = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
            want_steps += nsub
        elif what == 'birth':
            ks, ke = layers[arg]
            born = np.zeros(shape, dtype=bool)
            born[:, :, ks:ke + 1] = full[:, :, ks:ke + 1]
            T[born & ~mask] = Ts
            mask |= born
            grid.mask = mask.copy()
    assert nsteps == want_steps
    e = rel_linf(got, T)
    print('run_layer_birth with surface loss: %d steps, sub-steps per segment %s, rel L-inf %.3e' % (nsteps, nsubs, e))
    assert e <= 1e-10, e
    # the loss is at work: the constant-h loop with the law's h at ambient differs
    cold, _ = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), 12.0, Tinf, Ts, theta, cfl, layers, tb, t_out)
    assert rel_linf(cold, T) > 1e-3
    with pytest.raises(ValueError, match='device loop'):
        waam.run_layer_birth(hip, full, dx, (RHO, CP, K), 0.0, Tinf, Ts, theta, cfl, layers, tb, t_out, surface_loss=loss,
                             device_loop=False)


def test_run_single_track_with_surface_loss(mods):
    """waam.run_single_track: columns of 20 sub-steps (graph path) and, with a larger dt, of 4 (step by step), with and without
    the moving source, against the column loop written here over the oracle"""
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    shape, dx = (10, 9, 8), 1e-3
    plate = np.zeros(shape, dtype=bool)
    plate[:, :, :4] = True
    box = (3, 7, 4, 7, 3)                               # x0, x1, z0, z1, columns
    Tinf, T_track, theta, t_step = 25.0, 1500.0, 0.5, 0.4
    loss = hip.SurfaceLoss(h=10.0, emissivity=0.8)
    src0 = hip.GoldakSource(power=300.0, eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
    for dt, with_src in ((0.02, False), (0.1, True), (0.02, True)):
        got = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), 0.0, Tinf, T_track, theta, dt, t_step,
                                    heat_source=src0 if with_src else None, surface_loss=loss)
        x0, x1, z0, z1, ncol = box
        mask = plate.copy()
        grid, mat = orc.Grid3D(*shape, dx, mask), orc.Material(RHO, CP, K)
        T = np.full(shape, Tinf)
        n_sub = max(1, int(math.ceil(t_step / dt)))
        prm = orc.Params(t_step / n_sub, theta)
        for yi in range(ncol):
            mask[x0:x1, yi:yi + 1, z0:z1] = True
            grid.mask = mask.copy()
            T[x0:x1, yi:yi + 1, z0:z1] = T_track
            src = waam.track_source(src0, box, dx, yi, t_step) if with_src else None
            for i in range(n_sub):
                packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=slc.h_fields(loss, T, Tinf))
                if src is not None:
                    packs[0].qflux = packs[0].qflux + src.sample(grid, i * prm.dt + 0.5 * prm.dt) / (RHO * CP)
                T = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
        e = rel_linf(got, T)
        print('run_single_track dt %.3g source %s: %d sub-steps per column, rel L-inf %.3e' % (dt, with_src, n_sub, e))
        assert (n_sub >= waam.GRAPH_MIN_NSUB) == (dt == 0.02)
        assert e <= 1e-10, (dt, with_src, e)


# ---- physics: a small hot cube radiating into a cold void ----------------------------------------------------------------
def test_radiating_cube_follows_the_lumped_closed_form(mods):
    """4 x 4 x 4 cube of side L, conductivity raised to 5e4 W/m/K (Bi = h L / k about 2e-5: the cube is isothermal), emissivity
    0.8, no convection, field in kelvin (T_offset 0), ambient 1e-6 K (the law needs an ambient above 0 K; next to 1800 K it is
    0 K to 1e-9).  Lumped balance rho cp L^3 dT/dt = -6 L^2 eps sigma T^4:
        T(t) = (T0^-3 + 3 (6 eps sigma / (rho cp L)) t)^(-1/3).
    The scheme evaluates h at the start of each step, which is first order in dt.  The bar is the error of the SAME loop run
    through the C oracle on the CPU (backward Euler, t_end = 2 s, relative error of the mean temperature):
        dt = 0.1  s (20 steps): 1.3954e-3        dt = 0.05 s (40 steps): 6.9263e-4        ratio 2.0146
    The GPU result is within 1e-10 of the oracle's, so any factor above 1 holds; the test asserts twice those figures and a
    ratio between 1.6 and 2.4."""
    hip, _ = mods
    ORACLE_ERR = {20: 1.3954e-3, 40: 6.9263e-4}
    n, dx, k_hi, eps, T0, Tinf, t_end = 4, 1e-3, 5.0e4, 0.8, 1800.0, 1e-6, 2.0
    loss = hip.SurfaceLoss(h=0.0, emissivity=eps, T_offset=0.0)
    a = 6.0 * eps * loss.SIGMA / (RHO * CP * n * dx)
    exact = (T0 ** -3 + 3.0 * a * t_end) ** (-1.0 / 3.0)
    errs = {}
    for nst in (20, 40):
        grid = hip.Grid3D(n, n, n, dx, np.ones((n, n, n), dtype=bool))
        mat, prm = hip.Material(RHO, CP, k_hi), hip.Params(t_end / nst, 1.0)
        lp = hip.LossPacks(grid, mat, loss, Tinf)
        T = hip.StagedStepper(grid, mat, prm, lp.packs, Tinf, surface_loss=lp).run(hip.to_device(np.full((n, n, n), T0)), nst)
        T = np.asarray(T)
        assert (T.max() - T.min()) / T.mean() < 1e-4          # isothermal
        errs[nst] = abs(T.mean() - exact) / exact
        print('radiating cube: %d steps, mean T %.6f K, closed form %.6f K, relative error %.4e (oracle %.4e)'
              % (nst, T.mean(), exact, errs[nst], ORACLE_ERR[nst]))
    for nst in (20, 40):
        assert errs[nst] <= 2.0 * ORACLE_ERR[nst], (nst, errs[nst])
    assert 1.6 <= errs[20] / errs[40] <= 2.4, errs
