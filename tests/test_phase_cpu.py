"""CPU: the latent-heat law -- PhaseChange.correct, the NumPy definition of adi_phase_apply -- over the pinned C oracle against
the golden vectors of the reference (tests/golden/make_golden_phase.py), its conservation of enthalpy, the Stefan problem, and the
argument checks of the library, which run before any HIP call.

Bars: on the very T* a file stores, (T, f) np.array_equal (IEEE multiply / add / divide in one fixed order on both sides); whole
sequences T <= 1e-10 relative L-inf, the project's bar, and |f - f_golden| <= 1e-10 max|T| / (Tl - Ts), the same bar pushed
through f = (T - Ts)/dT (T and f are continuous in H across the branches)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import phase_cases as pc  # noqa: E402
from phase_cases import rel_linf  # noqa: E402


@pytest.fixture(scope='module')
def mods():
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


@pytest.mark.parametrize('name', pc.CASES)
def test_correct_is_the_golden_law_bit_for_bit(mods, name):
    hip, _ = mods
    c = pc.load(name)
    law = pc.law_of(c, hip.PhaseChange)
    dm, _ = pc.dir_of(c)
    mask = c['mask']
    assert np.array_equal(law.f_eq(c['T0']) * mask, c['f0'])
    f = c['f0']
    moved = 0
    for n in range(1, int(c['nsteps']) + 1):
        Tstar = c['Tstar%d' % n]
        T, fn = law.correct(Tstar, f, mask, dm, float(c['cp']))
        assert np.array_equal(T, c['T%d' % n]) and np.array_equal(fn, c['f%d' % n]), (name, n)
        keep = ~mask if dm is None else (~mask | dm)
        assert np.array_equal(T[keep], Tstar[keep]) and np.array_equal(fn[keep], f[keep])
        moved += int((T != Tstar).sum())
        f = c['f%d' % n]
    assert moved > 0
    if name == 'holes':
        assert c['counts'].tolist() == [550, 168, 25, 3, 1804]
        assert dm.any() and (c['f0'][dm] > 0).any() and (c['f0'][dm] < 1).any()     # Dirichlet cells in the freezing range


@pytest.mark.parametrize('name', pc.CASES)
def test_sequence_over_the_oracle(mods, name):
    hip, orc = mods
    c = pc.load(name)
    law = pc.law_of(c, hip.PhaseChange)
    worst = [0.0, 0.0]

    def visit(n, Tstar, T, f):
        eT, ef = rel_linf(T, c['T%d' % n]), float(np.abs(f - c['f%d' % n]).max())
        worst[0], worst[1] = max(worst[0], eT), max(worst[1], ef)
        assert eT <= 1e-10 and ef <= pc.f_bar(c), (name, n, eT, ef)
    pc.run_corrected(orc, c, law, visit)
    print(name, 'worst T rel L-inf %.3e, worst |df| %.3e (bar %.3e)' % (worst[0], worst[1], pc.f_bar(c)))


def test_enthalpy_is_conserved_on_the_adiabatic_holes_mask(mods):
    """the holes case without loss and without Dirichlet cells, 8 steps: the approximate factorisation conserves sum(T) (each
    1-D operator has zero column sums), the correction the enthalpy of each cell; the drift of sum(cp T + L f) over the mask is
    rounding, about 500 cells x 8 steps of it: bar 1e-12 relative"""
    hip, orc = mods
    c = pc.load('holes')
    law = pc.law_of(c, hip.PhaseChange)
    mask = np.array(c['mask'])
    cp, L = float(c['cp']), float(c['latent_heat'])
    grid = orc.Grid3D(*mask.shape, float(c['dx']), mask)
    mat = orc.Material(float(c['rho']), cp, float(c['k']))
    prm = orc.Params(float(c['seg0_dt']), float(c['theta']))
    packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=None)
    T = np.array(c['T0'])
    f = law.f_eq(T) * mask
    H0 = float(np.sum((cp * T + L * f)[mask]))
    branches = set()
    for _ in range(8):
        Tstar = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=25.0)
        T, f = law.correct(Tstar, f, mask, None, cp)
        branches |= {'solid' if (f[mask] == 0).any() else '', 'liquid' if (f[mask] == 1).any() else '',
                     'mushy' if ((f[mask] > 0) & (f[mask] < 1)).any() else ''}
        drift = abs(float(np.sum((cp * T + L * f)[mask])) - H0) / H0
        assert drift <= 1e-12, drift
    print('relative drift of the enthalpy after 8 steps %.3e' % drift)
    assert {'solid', 'liquid', 'mushy'} <= branches


def test_stefan_front_follows_neumanns_solution(mods):
    """1 x 1 x 300 cells of 0.1 mm, the wall cell held at 1725, the rest at 1125, melting at 1425 +- 0.5, theta = 0.5 at
    cfl 2, 452 steps (0.64 s).  The front, (sum of f beyond the wall cell + 1/2) dx, against 2 lambda sqrt(kappa t) with lambda
    from Neumann's transcendental equation.  Bar: one cell width, the resolution of a fixed-grid enthalpy method, over the last
    three quarters of the run (the first quarter resolves the front with a handful of cells).  Measured maximum over those steps
    over the C oracle: 0.497 cells (lambda = 0.331680, the front ends at 19.94 cells); it is printed."""
    hip, orc = mods
    s = pc.STEFAN
    law = hip.PhaseChange(s['latent'], s['T_melt'] - s['half_range'], s['T_melt'] + s['half_range'])
    lam = pc.stefan_lambda()
    shape, mask, T, dm, dv, dt = pc.stefan_setup(1)
    grid = orc.Grid3D(*shape, s['dx'], mask)
    mat = orc.Material(pc.RHO, pc.CP, pc.K)
    prm = orc.Params(dt, s['theta'])
    packs = orc.precompute_coeff_packs_unified(grid, mat, dir_mask=dm, dir_value=dv)
    f = law.f_eq(T) * mask
    worst = 0.0
    for n in range(1, s['nsteps'] + 1):
        Tstar = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=0.0)
        T, f = law.correct(Tstar, f, mask, dm, pc.CP)
        if 4 * n >= s['nsteps']:
            worst = max(worst, pc.stefan_front_error(f[0, 0], n, dt, lam))
    front = 2.0 * lam * np.sqrt(pc.KAPPA * s['nsteps'] * dt) / s['dx']
    print('lambda %.6f, front after %d steps at %.2f cells, worst error over the last three quarters %.3f cells'
          % (lam, s['nsteps'], front, worst))
    assert front > 15.0
    assert worst <= 1.0, worst


def test_law_validation():
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    assert law.key() == (2.7e5, 1400.0, 1450.0)
    assert law.constants(490.0) == (50.0, 490.0 * 1400.0, 490.0 * 1450.0 + 2.7e5, 490.0 + 2.7e5 / 50.0)
    assert np.array_equal(law.f_eq(np.array([0.0, 1400.0, 1425.0, 1450.0, 3000.0])), [0.0, 0.0, 0.5, 1.0, 1.0])
    for args, what in (((0.0, 1400.0, 1450.0), 'latent_heat'), ((-1.0, 1400.0, 1450.0), 'latent_heat'),
                       ((2.7e5, 1450.0, 1450.0), 'T_liquidus'), ((2.7e5, 1450.0, 1400.0), 'T_liquidus'),
                       ((float('nan'), 1400.0, 1450.0), 'non-finite'), ((2.7e5, 1400.0, float('inf')), 'non-finite'),
                       (('x', 1400.0, 1450.0), 'real numbers')):
        with pytest.raises(ValueError, match=what):
            hip.PhaseChange(*args)
    law.T_liquidus = 1300.0                               # a law broken after construction is caught where it is used
    with pytest.raises(ValueError, match='T_liquidus'):
        law.as_c()
    with pytest.raises(ValueError, match='cp'):
        hip.PhaseChange(2.7e5, 1400.0, 1450.0).constants(0.0)


def test_argument_errors_without_gpu():
    """adi_phase_apply / adi_phase_seed validate before any HIP call"""
    from adi_thermal_fields_amd import _lib
    P = ctypes.c_void_p(256)

    def law(L=2.7e5, Ts=1400.0, Tl=1450.0):
        return ctypes.byref(_lib.PhaseChangeLaw(L, Ts, Tl))

    def apply(law_=None, cp=490.0, T=P, f=ctypes.c_void_p(512), flags=P, summary=P, dims=(4, 4, 4, 0), null_law=False):
        return _lib.lib.adi_phase_apply(None if null_law else (law_ or law()), cp, T, f, flags, None, None, summary, *dims, None)

    def seed(law_=None, T=P, f=ctypes.c_void_p(512), flags=P, summary=P, dims=(4, 4, 4, 0), null_law=False):
        return _lib.lib.adi_phase_seed(None if null_law else (law_ or law()), T, f, flags, None, None, summary, *dims, None)
    for fn in (apply, seed):
        name = 'adi_phase_apply' if fn is apply else 'adi_phase_seed'
        for kw in (dict(null_law=True), dict(T=None), dict(f=None), dict(flags=None), dict(summary=None)):
            with pytest.raises(ValueError, match=name + ': null argument'):
                _lib.check(fn(**kw))
        with pytest.raises(ValueError, match='aliases'):
            _lib.check(fn(f=P))
        for bad, what in ((law(L=0.0), 'latent_heat must be > 0'), (law(L=-3.0), 'latent_heat must be > 0'),
                          (law(Ts=1450.0), 'T_liquidus must be above'), (law(Ts=1500.0), 'T_liquidus must be above'),
                          (law(L=float('nan')), 'latent_heat, T_solidus or T_liquidus not finite'),
                          (law(Tl=float('inf')), 'latent_heat, T_solidus or T_liquidus not finite')):
            with pytest.raises(ValueError, match=name + ': ' + what):
                _lib.check(fn(law_=bad))
        with pytest.raises(ValueError, match='bad grid'):
            _lib.check(fn(dims=(4, 0, 4, 0)))
        with pytest.raises(ValueError, match='plane_stride'):
            _lib.check(fn(dims=(4, 4, 4, 15)))
    for cp in (0.0, -490.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='adi_phase_apply: cp must be finite and > 0'):
            _lib.check(apply(cp=cp))
    assert _lib.lib.adi_phase_summary_words(20, 18, 35) == 2 * 2 * 3
    assert _lib.lib.adi_phase_summary_words(16, 16, 16) == 1 and _lib.lib.adi_phase_summary_words(0, 16, 16) == 0
