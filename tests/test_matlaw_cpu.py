"""CPU: temperature-dependent k(T) and cp(T) -- MaterialLaw, the NumPy definition of the kernels of csrc/adi_matlaw.hip -- in
the loop theta = Theta(T) -> linear step -> recover over the pinned C oracle: round trips and tables, validation, the reference's
golden vectors where the law degenerates to theirs, conservation of enthalpy, the bar problem, the Robin energy, and the argument
checks of the library and of the step, which run before any launch.

Bars: round trips 1e-13 max|T|; constant properties against the plain step 1e-12 relative; the latent-heat golden vectors the
project's 1e-10 on T and phase_cases.f_bar on f_eq(T); enthalpy drift 1e-12 relative; Robin energy 1e-12 relative."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import matlaw_cases as mc  # noqa: E402
import phase_cases as pc  # noqa: E402
from matlaw_cases import rel_linf  # noqa: E402


@pytest.fixture(scope='module')
def mods():
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


@pytest.fixture(scope='module')
def steel(mods):
    return mc.steel(mods[0].MaterialLaw)


# ---- round trips and tables ---------------------------------------------------------------------------------------------------
def _sample(law):
    return np.concatenate([np.linspace(-100.0, 3000.0, 62001), law.x, np.nextafter(law.x, -np.inf), np.nextafter(law.x, np.inf)])


@pytest.mark.parametrize('which', ['theta', 'enthalpy'])
def test_round_trip_over_the_whole_range(steel, which):
    """theta_inv(theta(T)) and enthalpy_inv(enthalpy(T)) over [-100, 3000], every knot and both linear ends included, within
    1e-13 max|T|.  Measured here: 4.547e-13 for both, one unit in the last place of a number in [2048, 4096)."""
    T = _sample(steel)
    fwd, inv = (steel.theta, steel.theta_inv) if which == 'theta' else (steel.enthalpy, steel.enthalpy_inv)
    err = np.abs(inv(fwd(T)) - T)
    print('%s round trip: worst %.3e at T = %.6f; worst below 2048: %.3e; samples off above 2048: %.1f %%'
          % (which, err.max(), T[err.argmax()], err[np.abs(T) < 2048].max(), 100.0 * (err[T >= 2048] > 0).mean()))
    assert np.array_equal(inv(fwd(steel.x)), steel.x)                       # the knots themselves are exact
    assert err.max() <= 1e-13 * np.abs(T).max(), err.max()


def test_tables_are_the_trapezoid_sums_of_the_knots(steel):
    law = steel
    x, kv = law.x, law.k_of(law.x)
    assert np.array_equal(x, [20.0, 400.0, 800.0, 1200.0, 1450.0, 1500.0, 2500.0]) and law.n == 7    # Ts, Tl are knots already
    th = x[0] + np.concatenate([[0.0], np.cumsum(0.5 * (kv[1:] + kv[:-1]) * np.diff(x))]) / law.k_ref
    assert rel_linf(law.th, th) <= 1e-14 and law.th[0] == x[0]
    cl = np.array(mc.STEEL_CP)
    boost = np.where((x[:-1] >= mc.STEEL_TS) & (x[1:] <= mc.STEEL_TL), mc.STEEL_L / (mc.STEEL_TL - mc.STEEL_TS), 0.0)
    H = cl[0] * x[0] + np.concatenate([[0.0], np.cumsum((0.5 * (cl[1:] + cl[:-1]) + boost) * np.diff(x))])
    assert rel_linf(law.H, H) <= 1e-14 and law.H[0] == 450.0 * 20.0
    assert abs((law.H[5] - law.H[4]) - (0.5 * (700.0 + 800.0) * 50.0 + 2.7e5)) <= 1e-9          # the latent heat is all there
    # the defaults, and the held ends
    assert law.k_ref == 52.0 and law.cp_ref == law.c_eff_min == min(c * 52.0 / k for c, k in zip(mc.STEEL_CP, mc.STEEL_K))
    assert law.min_theta() == 0.5
    assert np.allclose(law.k_of([-500.0, 20.0, 210.0, 2500.0, 9000.0]), [52.0, 52.0, 48.0, 60.0, 60.0], rtol=1e-15, atol=0.0)
    assert np.array_equal(law.cp_of([-500.0, 20.0, 210.0, 1500.0, 9000.0]), [450.0, 450.0, 505.0, 800.0, 800.0])
    assert law.cp_of(1450.0) == 700.0 + 5400.0 and law.cp_of(np.nextafter(1450.0, 0.0)) < 701.0    # cp jumps at the solidus
    assert np.array_equal(law.f_eq([0.0, 1450.0, 1475.0, 1500.0, 3000.0]), [0.0, 0.0, 0.5, 1.0, 1.0])
    # beyond the end knots both maps are linear
    assert law.theta(-80.0) == 20.0 + 1.0 * (-100.0) and law.enthalpy(-80.0) == 9000.0 + 450.0 * (-100.0)
    m = law.material(7800.0)
    assert (m.rho, m.cp, m.k) == (7800.0, law.cp_ref, 52.0)
    assert law.key() == mc.steel(type(law)).key() != mc.steel(type(law), cp_ref=400.0).key()


def test_latent_points_are_merged_into_the_knots(mods):
    hip, _ = mods
    law = hip.MaterialLaw([0.0, 1000.0, 2000.0], [50.0, 30.0, 40.0], [500.0, 700.0, 600.0], 2.0e5, 1400.0, 1440.0)
    assert np.array_equal(law.x, [0.0, 1000.0, 1400.0, 1440.0, 2000.0])
    assert np.allclose(law.k_of(law.x), [50.0, 30.0, 34.0, 34.4, 40.0], rtol=1e-15, atol=0.0)
    assert law.cp_of(1400.0) == 660.0 + 5000.0 and law.cp_of(1440.0) == 656.0 and law.cp_of(1399.0) < 661.0
    assert law.c_eff_min == 500.0                                           # before the boost
    T = np.linspace(-50.0, 2100.0, 4001)
    assert np.abs(law.enthalpy_inv(law.enthalpy(T)) - T).max() <= 1e-12 and (np.diff(law.enthalpy(T)) > 0).all()
    # the latent interval may lie outside the given knots: k and cp are held there
    out = hip.MaterialLaw([0.0, 100.0], [50.0, 30.0], [500.0, 700.0], 2.0e5, 150.0, 160.0)
    assert np.array_equal(out.x, [0.0, 100.0, 150.0, 160.0]) and out.cp_of(155.0) == 700.0 + 2.0e4 and abs(out.k_of(155.0) - 30.0) < 1e-13


def test_constructor_validation(mods):
    hip, _ = mods
    L = hip.MaterialLaw
    T, k, cp = [0.0, 100.0, 200.0], [50.0, 40.0, 30.0], [400.0, 500.0, 600.0]
    L(T, k, cp)
    for args, kw, what in (
            (([0.0], [50.0], [400.0]), {}, 'at least 2 knots'),
            ((T, k[:2], cp), {}, 'as many k and cp'),
            ((T, k, cp[:2]), {}, 'as many k and cp'),
            (([0.0, 100.0, 100.0], k, cp), {}, 'do not increase'),
            (([0.0, 200.0, 100.0], k, cp), {}, 'do not increase'),
            ((T, [50.0, 0.0, 30.0], cp), {}, 'must be > 0'),
            ((T, k, [400.0, -1.0, 600.0]), {}, 'must be > 0'),
            ((T, [50.0, float('nan'), 30.0], cp), {}, 'non-finite'),
            (([0.0, 100.0, float('inf')], k, cp), {}, 'non-finite'),
            ((T, 'abc', cp), {}, 'real numbers'),
            ((T, k, cp), dict(latent_heat=1e5), 'come together'),
            ((T, k, cp), dict(T_solidus=50.0, T_liquidus=60.0), 'come together'),
            ((T, k, cp), dict(latent_heat=0.0, T_solidus=50.0, T_liquidus=60.0), 'latent_heat'),
            ((T, k, cp), dict(latent_heat=1e5, T_solidus=60.0, T_liquidus=60.0), 'T_liquidus'),
            ((T, k, cp), dict(k_ref=0.0), 'k_ref'),
            ((T, k, cp), dict(cp_ref=float('inf')), 'cp_ref'),
            ((list(range(17)), [50.0] * 17, [400.0] * 17), {}, 'more than 16 knots'),
            ((list(range(15)), [50.0] * 15, [400.0] * 15), dict(latent_heat=1e5, T_solidus=0.5, T_liquidus=1.5),
             'more than 16 knots after merging')):
        with pytest.raises(ValueError, match=what):
            L(*args, **kw)
    assert L(list(range(14)), [50.0] * 14, [400.0] * 14, 1e5, 0.5, 1.5).n == 16 == L.MAX_KNOTS
    # cp_ref above the default raises the smallest stable theta
    law = L(T, k, cp, cp_ref=600.0)
    assert law.c_eff_min == 400.0 and law.min_theta() == 0.75


class _Stub:
    pass


def test_check_extras_refuses_before_any_launch(mods, steel):
    """the checks of `material=` run in _check_extras, ahead of the first launch: here without a GPU, on a NonlinearPacks put
    together by hand"""
    hip, _ = mods
    from adi_thermal_fields_amd import step
    grid, packs = _Stub(), (_Stub(), _Stub(), _Stub())
    nm = object.__new__(hip.NonlinearPacks)
    nm.grid, nm.packs, nm._law, nm.mat = grid, packs, steel, steel.material(7800.0)
    prm = hip.Params(0.01, 0.5)

    def check(grid=grid, mat=nm.mat, prm=prm, packs=packs, surface_loss=None, phase=None, material=nm):
        step._check_extras(grid, mat, prm, packs, step.StepExtras(surface_loss=surface_loss, phase=phase, material=material))
    check()
    with pytest.raises(TypeError, match='NonlinearPacks'):
        check(material=steel)
    with pytest.raises(ValueError, match='own packs'):
        check(packs=(packs[0], packs[1], _Stub()))
    with pytest.raises(ValueError, match='own material'):
        check(mat=hip.Material(7800.0, 490.0, 52.0))
    with pytest.raises(ValueError, match='own material'):
        check(mat=hip.Material(7700.0, nm.mat.cp, nm.mat.k))
    with pytest.raises(ValueError, match='cannot be combined'):
        check(phase=_Stub())
    with pytest.raises(ValueError, match='cannot be combined'):
        check(surface_loss=_Stub())
    with pytest.raises(ValueError, match='stability limit'):
        check(prm=hip.Params(0.01, 0.49))
    with pytest.raises(ValueError, match='another grid'):
        check(grid=_Stub())
    # cp_ref = 2 min c_eff is stable from theta = 1 on
    nm._law = mc.steel(hip.MaterialLaw, cp_ref=900.0)
    nm.mat = nm.law.material(7800.0)
    assert nm.law.min_theta() == 1.0
    check(mat=nm.mat, prm=hip.Params(0.01, 1.0))
    with pytest.raises(ValueError, match='stability limit'):
        check(mat=nm.mat, prm=hip.Params(0.01, 0.5))


def test_argument_errors_without_gpu(steel):
    """adi_matlaw_theta / adi_matlaw_recover / adi_matlaw_loss_update validate before any HIP call"""
    from adi_thermal_fields_amd import _lib
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    P, Q = ctypes.c_void_p(256), ctypes.c_void_p(512)
    loss = hip.SurfaceLoss(h=10.0).as_c(20.0)
    coeff = _lib.ptr_array([256, 512, 768])

    def law(**kw):
        w = steel.as_c()
        for name, (i, v) in kw.items():
            if i is None:
                setattr(w, name, v)
            else:
                getattr(w, name)[i] = v
        return ctypes.byref(w)

    def theta(law_=None, T=P, out=Q, flags=P, dims=(4, 4, 4, 0), null_law=False):
        return _lib.lib.adi_matlaw_theta(None if null_law else (law_ or law()), T, out, flags, None, *dims, None)

    def recover(law_=None, T=P, out=Q, flags=P, dims=(4, 4, 4, 0), null_law=False):
        return _lib.lib.adi_matlaw_recover(None if null_law else (law_ or law()), T, out, flags, None, None, *dims, None)

    def update(law_=None, T=P, out=coeff, flags=P, dims=(4, 4, 4, 0), null_law=False, Tinf=20.0, k=(0, 4), cp=450.0):
        return _lib.lib.adi_matlaw_loss_update(None if null_law else (law_ or law()), ctypes.byref(loss), Tinf, T, flags, None,
                                               *dims, 1e-3, 7800.0, cp, out, k[0], k[1], 0, None)
    for fn, name in ((theta, 'adi_matlaw_theta'), (recover, 'adi_matlaw_recover'), (update, 'adi_matlaw_loss_update')):
        for kw in (dict(null_law=True), dict(T=None), dict(out=None), dict(flags=None)):
            with pytest.raises(ValueError, match=name + ': null argument'):
                _lib.check(fn(**kw))
        for bad, what in ((law(n_knots=(None, 1)), '2 to 16 knots'), (law(n_knots=(None, 17)), '2 to 16 knots'),
                          (law(k_ref=(None, 0.0)), 'k_ref, cp_ref and c_lo'), (law(cp_ref=(None, float('nan'))), 'k_ref, cp_ref'),
                          (law(c_lo=(None, -1.0)), 'k_ref, cp_ref and c_lo'), (law(x=(2, float('inf'))), 'not finite at knot 2'),
                          (law(kq=(3, 0.0)), r'must be > 0 \(knot 3\)'), (law(c=(1, -2.0)), r'must be > 0 \(knot 1\)'),
                          (law(x=(2, 300.0)), 'do not increase at knot 2'), (law(theta=(4, 100.0)), 'do not increase at knot 4'),
                          (law(H=(6, 0.0)), 'do not increase at knot 6'), (law(hks=(6, 1e-3)), 'last piece'),
                          (law(ks2=(1, -1.0)), 'disagree on the interval below knot 2')):
            with pytest.raises(ValueError, match=name + ': .*' + what):
                _lib.check(fn(law_=bad))
        with pytest.raises(ValueError, match='bad grid'):
            _lib.check(fn(dims=(4, 0, 4, 0)))
        with pytest.raises(ValueError, match='plane_stride'):
            _lib.check(fn(dims=(4, 4, 4, 15)))
    for fn in (theta, recover):
        with pytest.raises(ValueError, match='aliases'):
            _lib.check(fn(out=P))
    with pytest.raises(ValueError, match='adi_matlaw_loss_update: bad plane range'):
        _lib.check(update(k=(2, 9)))
    with pytest.raises(ValueError, match='adi_matlaw_loss_update: dx, rho and cp'):
        _lib.check(update(cp=0.0))
    with pytest.raises(ValueError, match='adi_matlaw_loss_update: Tinf not finite'):
        _lib.check(update(Tinf=float('nan')))
    with pytest.raises(ValueError, match='ambient in kelvin'):
        _lib.check(update(Tinf=-300.0))
    # the unchanged entry still names itself
    with pytest.raises(ValueError, match='adi_surface_loss_update: bad plane range'):
        _lib.check(_lib.lib.adi_surface_loss_update(ctypes.byref(loss), 20.0, P, P, None, 4, 4, 4, 0, 1e-3, 7800.0, 450.0, coeff, 2, 9,
                                                    0, None))


# ---- against the reference's golden vectors ------------------------------------------------------------------------------
def test_constant_properties_are_the_plain_step(mods):
    """k and cp constant, no latent heat: Theta(T) = T and H = cp T up to rounding, the ratio is 1, and the loop is the
    reference's step: holes_mixed (every kind of boundary condition, theta = 1) to 1e-12 relative at every step"""
    hip, orc = mods
    import cases
    c = cases.cart_case('holes_mixed')
    m = c['mat']
    law = hip.MaterialLaw([20.0, 700.0, 1500.0], [m['k']] * 3, [m['cp']] * 3)
    assert (law.k_ref, law.cp_ref, law.min_theta()) == (m['k'], m['cp'], 0.5)
    grid = orc.Grid3D(*c['shape'], c['dx'], c['mask'])
    mat, prm = orc.Material(**m), orc.Params(c['dt'], c['theta'])
    packs = orc.precompute_coeff_packs_unified(grid, mat, dir_mask=c['dir_mask'], dir_value=c['dir_value'], neumann=c['neumann'],
                                               robin_h=c['robin_h'])
    shape = c['shape']
    a = b = c['T0']
    for n in range(c['nsteps']):
        a = orc.adi_step_numba_coeff(a, grid, mat, prm, packs, Tinf=c['Tinf'])
        r = law.robin_ratio(b, c['Tinf'])
        robin = {f: (np.full(shape, h) if np.isscalar(h) else h) * r for f, h in c['robin_h'].items()}
        b, _, _ = mc.loop_step(orc, law, grid, prm, b, c['Tinf'], rho=m['rho'], robin=robin, dm=c['dir_mask'], dv=c['dir_value'],
                               neumann=c['neumann'])
        e = rel_linf(b, a)
        print('step', n + 1, 'rel L-inf %.3e' % e)
        assert e <= 1e-12, (n, e)
        assert np.array_equal(b[~c['mask']], c['T0'][~c['mask']])


@pytest.mark.parametrize('name', pc.CASES)
def test_constant_properties_with_latent_heat_are_the_phase_golden_vectors(mods, name):
    """k and cp constant plus latent heat: the stateless law is PhaseChange's when f = f_eq(T), which the golden runs keep; T<n>
    to the project's 1e-10 on every cell, f_eq(T) against f<n> at phase_cases.f_bar on every cell whose f the reference's law
    moves: a Dirichlet cell keeps the f it was seeded with while its T becomes the held value (PhaseChange.correct leaves it
    alone), so there f<n> is not f_eq(T<n>) in the golden vectors themselves -- that is asserted too"""
    hip, orc = mods
    c = pc.load(name)
    Ts, Tl = float(c['T_solidus']), float(c['T_liquidus'])
    law = hip.MaterialLaw([Ts - 900.0, Tl + 700.0], [float(c['k'])] * 2, [float(c['cp'])] * 2, float(c['latent_heat']), Ts, Tl)
    assert law.cp_ref == float(c['cp']) and float(c['theta']) >= law.min_theta()
    mask = np.array(c['mask'])
    grid = orc.Grid3D(*mask.shape, float(c['dx']), mask)
    dm, dv = pc.dir_of(c)
    T, Tinf = np.array(c['T0']), float(c['Tinf'])
    loss = hip.SurfaceLoss(h=float(c['h']))
    n, worst = 0, [0.0, 0.0]
    free = mask if dm is None else mask & ~dm
    for dt, nsteps, S in pc.segments(c):
        prm = orc.Params(dt, float(c['theta']))
        for _ in range(nsteps):
            T, _, _ = mc.loop_step(orc, law, grid, prm, T, Tinf, rho=float(c['rho']), robin=mc.robin_fields(law, loss, T, Tinf),
                                   dm=dm, dv=dv, S=S)
            n += 1
            eT, ef = rel_linf(T, c['T%d' % n]), float(np.abs(law.f_eq(T) - c['f%d' % n])[free].max())
            if dm is not None:
                assert np.array_equal(c['f%d' % n][dm], c['f0'][dm])
            worst = [max(worst[0], eT), max(worst[1], ef)]
            assert eT <= 1e-10 and ef <= pc.f_bar(c), (name, n, eT, ef)
    assert n == int(c['nsteps'])
    print(name, 'worst T rel L-inf %.3e, worst |f_eq(T) - f| %.3e (bar %.3e)' % (worst[0], worst[1], pc.f_bar(c)))


# ---- physics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('theta', [0.5, 1.0])
def test_enthalpy_is_conserved_on_the_adiabatic_holes_mask(mods, steel, theta):
    """no loss, no Dirichlet cell, 8 steps from a field that spans the table: each 1-D operator has zero column sums, so the linear
    step conserves sum(Theta), and the recovery adds cp_ref times each cell's change of Theta to its enthalpy; the drift of
    sum(H(T)) over the mask is rounding: bar 1e-12 relative"""
    hip, orc = mods
    mask = mc.holes_mask()
    assert mask.shape == (9, 7, 11)
    rng = np.random.default_rng(17)
    T = np.where(mask, rng.uniform(300.0, 2200.0, mask.shape), 25.0)
    dx = 5e-4
    grid = orc.Grid3D(*mask.shape, dx, mask)
    prm = orc.Params(4.0 * dx * dx * mc.RHO * steel.cp_ref / steel.k_ref, theta)
    H0 = float(np.sum(steel.enthalpy(T)[mask]))
    seen = set()
    for _ in range(8):
        T, _, _ = mc.loop_step(orc, steel, grid, prm, T, 25.0)
        f = steel.f_eq(T)[mask]
        seen |= {'solid' if (f == 0).any() else '', 'liquid' if (f == 1).any() else '', 'mushy' if ((f > 0) & (f < 1)).any() else ''}
        drift = abs(float(np.sum(steel.enthalpy(T)[mask])) - H0) / H0
        assert drift <= 1e-12, drift
    print('theta %.1f: relative drift of the enthalpy after 8 steps %.3e' % (theta, drift))
    assert {'solid', 'liquid', 'mushy'} <= seen


@pytest.mark.parametrize('theta', [0.5, 1.0])
def test_bar_is_monotone_and_converges(mods, steel, theta):
    """1 x 1 x 200 cells of 0.2 mm, the wall held at 2000, the bulk at 20, 0.5 s: the profile is monotone and stays within
    [20, 2000], both up to the rounding of a step (matlaw_cases.BAR_SLACK: the cells still at 20 move by a few 1e-14); against
    the fine explicit enthalpy integration of the same spatial scheme the error at 400 steps is at most half
    the error at 100 steps (first order in dt would give a quarter); the figures are printed"""
    _, orc = mods
    ref = mc.bar_reference(steel)
    errs = {}
    for nsteps in (100, 400):
        T = mc.bar_run(orc, steel, nsteps, theta)[0, 0]
        assert (np.diff(T) <= mc.BAR_SLACK).all() and T.min() >= 20.0 - mc.BAR_SLACK and T.max() <= 2000.0 + mc.BAR_SLACK, nsteps
        errs[nsteps] = float(np.abs(T - ref).max())
    print('theta %.1f: error %.2f K at 100 steps, %.2f K at 400 steps, ratio %.2f' % (theta, errs[100], errs[400],
                                                                                     errs[400] / errs[100]))
    assert (np.diff(ref) <= mc.BAR_SLACK).all() and ref[20] > 300.0                 # the heat has gone deep
    assert errs[400] <= 0.5 * errs[100], errs


def test_robin_sink_carries_the_loss_as_energy(mods, steel):
    """the stored coefficient times (Theta - Theta_inf) times Ccell is h(T) A (T - Tinf) summed over the exposed faces of the
    axis: 1e-12 relative wherever |T - Tinf| >= 1"""
    hip, orc = mods
    mask = mc.holes_mask()
    dx, Tinf = 5e-4, 25.0
    T = mc.field_over_the_law(steel, mask)
    sel = mask & (np.abs(T - Tinf) >= 1.0)
    loss = hip.SurfaceLoss(h={'x-': 15.0, 'x+': 0.0, 'y-': 40.0, 'y+': 8.0, 'z-': 0.0, 'z+': 120.0}, emissivity=0.7,
                           table=([0.0, 1000.0, 2000.0], [0.0, 30.0, 90.0]))
    grid = orc.Grid3D(*mask.shape, dx, mask)
    mat = orc.Material(mc.RHO, steel.cp_ref, steel.k_ref)
    packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=mc.robin_fields(steel, loss, T, Tinf))
    Ccell, A = mc.RHO * steel.cp_ref * dx ** 3, dx * dx
    dth = steel.theta(T) - steel.theta(Tinf)
    worst = 0.0
    for a in range(3):
        want = sum(np.where(orc.exposed_mask(mask, f), loss.h_of(T, f, Tinf) * A * (T - Tinf), 0.0) for f in mc.FACES[2 * a:2 * a + 2])
        got = packs[a].coeff * dth * Ccell
        on = sel & (want != 0.0)
        assert on.sum() > 20
        worst = max(worst, float(np.max(np.abs(got[on] - want[on]) / np.abs(want[on]))))
    print('Robin energy: worst relative difference %.3e' % worst)
    assert worst <= 1e-12
    # at the ambient itself the ratio is 1 / kq(Tinf), the limit
    assert abs(steel.robin_ratio(np.array([Tinf]), Tinf)[0] * steel.k_of(Tinf) / steel.k_ref - 1.0) <= 1e-15
    assert abs(steel.robin_ratio(np.array([Tinf + 1e-7]), Tinf)[0] * steel.k_of(Tinf) / steel.k_ref - 1.0) < 1e-6
