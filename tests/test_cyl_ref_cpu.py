"""CPU: the float64 oracle (oracle/cyl_oracle.py) measured against the extended-precision reference tests/cyl_ref_ld.py on
every case of the time-step sweep of tests/test_cyl_switches_gpu.py, and the reference pinned to the golden vectors.

The GPU bar is 1e-10 (BASELINE.json).  The oracle has to sit within a tenth of it, 1e-11, of the long-double result on every
case, so that its own rounding can neither hide nor cause a failure of the sweep; the measured figures are in DESIGN.md
("Cylindrical kernels: what reaches what")."""
import types

import numpy as np
import pytest

import cart_dt_cases as cd
import cases
import cyl_ref_ld
import cyl_switch_cases as csc
from helpers import golden, rel_linf, run_cyl_case
from oracle import cyl_oracle


@pytest.mark.parametrize('tag,key', csc.dt_params(), ids=[t for t, _ in csc.dt_params()])
def test_oracle_within_a_tenth_of_the_gpu_bar_of_the_long_double_reference(tag, key):
    shape, R_in, f = key
    _, want = csc.dt_reference(*key)
    got = csc.run_case(cyl_oracle, csc.dt_case(*key))
    err = rel_linf(got, want)
    print('oracle vs long double: %-44s %.3e' % (tag, err))
    assert np.all(np.isfinite(got))
    assert err <= 1e-11, (tag, err)
    # the increment metric of cart_dt_cases: the oracle within a quarter of the bar the GPU sweep is held to
    f = cd.cyl_figures(got, key)
    print('%22s inc %.2e K  err %.2e K = %6.2f ulp = %.1e inc' % ('', f['inc'], f['abs_err'], f['ulp'], f['of_inc']))
    assert f['abs_err'] <= cd.bar(f, cd.A_CYL / 4), (tag, f)
    _ULP[key] = f['ulp']


_ULP = {}


def test_recorded_cyl_oracle_worst_is_the_measured_one():
    """A_CYL as A of cart_dt_cases: 4 x the oracle's worst error at f <= 1e-3 in units of eps64 max|W|, rounded up to 2^n; the
    recorded worst is not below the measured one and not above twice it"""
    ks = [key for _, key in csc.dt_params() if key[2] <= 1e-3]
    for key in ks:
        if key not in _ULP:
            _ULP[key] = cd.cyl_figures(csc.run_case(cyl_oracle, csc.dt_case(*key)), key)['ulp']
    worst = max(_ULP[key] for key in ks)
    print('worst cylindrical oracle error at f <= 1e-3: %.3f eps64 max|W|; recorded %.3f, A_CYL = %g'
          % (worst, cd.CYL_ORACLE_WORST_ULP, cd.A_CYL))
    assert worst <= cd.CYL_ORACLE_WORST_ULP <= 2.0 * worst, (worst, cd.CYL_ORACLE_WORST_ULP)
    assert cd.A_CYL == cd.bar_factor(cd.CYL_ORACLE_WORST_ULP)


class _LdApi:
    """cyl_ref_ld behind the operator surface run_cyl_case drives (plain attribute holders for the five argument objects)"""
    @staticmethod
    def GridCyl(nr, nphi, nz, dr, dphi, dz, R, R_in=0.0):
        return types.SimpleNamespace(nr=nr, nphi=nphi, nz=nz, dr=dr, dphi=dphi, dz=dz, R=R, R_in=R_in)

    Material = staticmethod(lambda rho, cp, k: types.SimpleNamespace(rho=rho, cp=cp, k=k))
    Params = staticmethod(lambda dt, theta=0.5, scheme="be": types.SimpleNamespace(dt=dt))
    RobinR = staticmethod(lambda h, T_inf: types.SimpleNamespace(h=h, T_inf=T_inf))

    @staticmethod
    def ZBC(kind_bot='neumann0', kind_top='robin', h_bot=0.0, h_top=0.0, T_inf_bot=20.0, T_inf_top=20.0, T_bot=20.0, T_top=20.0):
        return types.SimpleNamespace(kind_bot=kind_bot, kind_top=kind_top, h_bot=h_bot, h_top=h_top, T_inf_bot=T_inf_bot,
                                     T_inf_top=T_inf_top, T_bot=T_bot, T_top=T_top)

    adi_step = staticmethod(cyl_ref_ld.adi_step)
    adi_step_masked = staticmethod(cyl_ref_ld.adi_step_masked)


@pytest.mark.parametrize('name', ['kat3', 'nphi36_masked', 'zbc_dirichlet_robin', 'zbc_robin_dirichlet', 'nphi2_source'])
def test_long_double_reference_reproduces_the_golden_vectors(name):
    """kat3 and nphi36_masked pin the reference to the golden vectors; the three others add what those two do not contain: a
    Dirichlet end at either side, two phi cells, a source field, no Robin at the outer radius"""
    g = golden('cyl', name)
    out = run_cyl_case(_LdApi, cases.cyl_case(name))
    for key in ('T_step1', 'T_final'):
        err = rel_linf(out[key].astype(np.float64), g[key])
        assert err <= 1e-12, (name, key, err)


@pytest.mark.parametrize('n', [2, 3, 4, 17, 64])
@pytest.mark.parametrize('f_r', [1e-13, 0.3, 1e6])
def test_periodic_solve_leaves_no_residual(n, f_r):
    """solve_phi against the periodic system written out row by row (no elimination): the residual stays at the rounding of
    np.longdouble times the size of the coefficients, at phi factors up to 1e6 * (1/(1.5 * 2 pi / 64))^2 ~ 5e7"""
    rng = np.random.default_rng(n)
    grid = types.SimpleNamespace(nr=3, nphi=n, nz=2, dr=csc.DR, dphi=2.0 * np.pi / n, dz=csc.DZ, R_in=0.0)
    mat = types.SimpleNamespace(**csc.STEEL)
    dt = f_r * csc.DR ** 2 / csc.ALPHA
    d = rng.uniform(20.0, 1200.0, (3, n, 2))
    x = cyl_ref_ld.solve_phi(d, grid, mat, dt)
    assert np.array_equal(x[0], d[0].astype(np.longdouble))          # fac_0 = 0: the axis row is an identity
    fmax = f_r / (1.5 * grid.dphi) ** 2
    assert cyl_ref_ld.residual(x, d, grid, mat, dt) <= 64 * float(np.finfo(np.longdouble).eps) * (1.0 + 4.0 * fmax)
