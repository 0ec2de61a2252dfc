"""CPU: the weights of the uniform axis-0 line of the slab decomposition (adi_axis0_weights_host: host arithmetic, the
builder of csrc/adi_axis0_weights.hpp that adi_axis0_dots_setup and adi_axis0_deferred_setup upload from).

    w = c * tridiag(-tg, 1+2tg, -tg)^-1 e_0,   tg = theta * gam,   c = 1 (dots) or c = tg (deferred)

1. Both kinds are, bit for bit, the same Thomas recurrence restated here in np.longdouble and rounded to float64.
2. Independently of the recurrence, its long-double solution leaves a residual max|A x - c e_0| of at most
   64 eps_longdouble (1 + 4 tg): the bound form of tests/test_cyl_ref_cpu.py.
3. w decreases monotonically; with tol = SlabStepper.DECAY_TOL every entry at or beyond `reach` is exactly 0 and every entry
   before it exceeds tol; tol = 0 cuts nothing.
4. The dense np.linalg.solve of tests/cpu_engine.py (CpuEngine.deferred_setup, which stays independent of the product) agrees:
   its own error against the long-double reference, max_i |w_dense[i] - x[i]| / x[0] over the cases below, was measured as
   1.823e-15 (n = 64, tg = 200; 1.1e-16 at tg = 1e-12, 1.1e-16 at tg = 0.15).  The margin is twice that: the library's
   weights lie within it of the dense ones, and so does the dense solve of the reference (LAPACK builds differ in their
   last bits).  The library's own output plays no part in the margin.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: a process that loads libadi_hip.so ahead of torch ends up with two HIP runtimes,
#                            and the GPU tests collected after this module share its process)

from adi_thermal_fields_amd import _lib
from adi_thermal_fields_amd.dist_slab import SlabStepper
from cpu_engine import CpuEngine

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "needs an extended-precision np.longdouble (x87: 64-bit significand)"

NS = (2, 3, 17, 64, 1024)
TGS = (1e-12, 0.15, 200.0)
THETA = 0.5                                  # theta * gam is exact: gam = 2 tg
DOTS, DEFERRED = 0, 1                        # ADI_AXIS0_WEIGHTS_DOTS / _DEFERRED of include/adi_hip.h
DENSE_ERR = 1.823e-15                        # measured, see the module's docstring
MARGIN = 2.0 * DENSE_ERR
CASES = [(n, tg) for n in NS for tg in TGS]


def _lib_weights(n, tg, kind, tol):
    w, reach = np.full(n, np.nan), ctypes.c_int(-1)
    _lib.check(_lib.lib.adi_axis0_weights_host(n, THETA, tg / THETA, kind, tol, w.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.byref(reach)))
    return w, reach.value


def _thomas_ld(n, tg, kind):
    """the builder's recurrence in np.longdouble: Thomas on c * e_0, operation for operation"""
    tg = LD(THETA) * LD(tg / THETA)
    b = LD(1) + LD(2) * tg
    c = tg if kind == DEFERRED else LD(1)
    cp, x = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    piv = b
    cp[0] = -tg / piv
    x[0] = c / piv
    for i in range(1, n):
        piv = b + tg * cp[i - 1]
        cp[i] = -tg / piv
        x[i] = (tg * x[i - 1]) / piv
    for i in range(n - 2, -1, -1):
        x[i] -= cp[i] * x[i + 1]
    return x, tg, c


@pytest.fixture(scope='module')
def reference():
    """{(n, tg, kind): (long-double solution, tg, c)}, computed once"""
    return {(n, tg, kind): _thomas_ld(n, tg, kind) for n, tg in CASES for kind in (DOTS, DEFERRED)}


@pytest.mark.parametrize('kind', [DOTS, DEFERRED], ids=['dots', 'deferred'])
@pytest.mark.parametrize('n,tg', CASES)
def test_weights_are_the_long_double_recurrence_rounded(reference, n, tg, kind):
    w, reach = _lib_weights(n, tg, kind, 0.0)
    x = reference[n, tg, kind][0]
    assert np.array_equal(w, x.astype(np.float64))
    assert reach == int(np.count_nonzero(w))              # tol = 0 cuts nothing: only entries that rounded to 0 are "cut"
    assert np.all(w[:reach] > 0.0) and np.all(w[reach:] == 0.0)


@pytest.mark.parametrize('kind', [DOTS, DEFERRED], ids=['dots', 'deferred'])
@pytest.mark.parametrize('n,tg', CASES)
def test_the_recurrence_solves_the_system(reference, n, tg, kind):
    x, tgl, c = reference[n, tg, kind]
    r = (LD(1) + LD(2) * tgl) * x
    r[1:] -= tgl * x[:-1]
    r[:-1] -= tgl * x[1:]
    r[0] -= c
    res = float(np.max(np.abs(r)))
    bound = 64 * float(np.finfo(LD).eps) * (1.0 + 4.0 * tg)
    print('n = %d, tg = %g, kind %d: residual %.3e, bound %.3e' % (n, tg, kind, res, bound))
    assert res <= bound


@pytest.mark.parametrize('kind', [DOTS, DEFERRED], ids=['dots', 'deferred'])
@pytest.mark.parametrize('n,tg', CASES)
def test_weights_decrease_and_the_cut_is_exact(n, tg, kind):
    w, reach = _lib_weights(n, tg, kind, 0.0)
    assert reach >= 1 and np.all(np.diff(w) <= 0.0)
    assert np.all(np.diff(w[:reach]) < 0.0)                # strictly, as far as the weights are non-zero
    tol = SlabStepper.DECAY_TOL
    wc, rc = _lib_weights(n, tg, kind, tol)
    assert 0 <= rc <= n
    assert np.all(wc[rc:] == 0.0) and np.all(wc[:rc] > tol)
    assert np.array_equal(wc[:rc], w[:rc]) and np.all(w[rc:] <= tol)


def test_bad_arguments_are_refused():
    w, reach = np.zeros(4), ctypes.c_int(0)
    pw, pr = w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(reach)
    f = _lib.lib.adi_axis0_weights_host
    assert f(1, THETA, 0.3, DEFERRED, 0.0, pw, pr) == _lib.ADI_ERR_ARG
    assert f(4, THETA, 0.3, DEFERRED, 0.0, None, pr) == _lib.ADI_ERR_ARG
    assert f(4, THETA, 0.3, DEFERRED, 0.0, pw, None) == _lib.ADI_ERR_ARG
    assert f(4, THETA, 0.3, DEFERRED, -1.0, pw, pr) == _lib.ADI_ERR_ARG
    assert f(4, THETA, 0.3, 2, 0.0, pw, pr) == _lib.ADI_ERR_ARG
    with pytest.raises(ValueError, match='adi_axis0_weights_host'):
        _lib.check(f(1, THETA, 0.3, DOTS, 0.0, pw, pr))
    assert f(4, THETA, 0.3, DEFERRED, 0.0, pw, pr) == _lib.ADI_OK


def test_the_dense_solve_of_the_cpu_engine_agrees(reference):
    """CpuEngine.deferred_setup (np.linalg.solve, tol = 0) against the long-double reference and against the library, both
    relative to the largest weight and within MARGIN = twice the dense solve's measured error"""
    worst = 0.0
    for n, tg in CASES:
        x = reference[n, tg, DEFERRED][0]
        dense = CpuEngine().deferred_setup(n, THETA, tg / THETA, 0.0)['w'].numpy()
        err = float(np.max(np.abs(dense.astype(LD) - x)) / x[0])
        worst = max(worst, err)
        print('n = %d, tg = %g: dense solve off the long-double reference by %.3e of w[0]' % (n, tg, err))
        assert err <= MARGIN
        w, _ = _lib_weights(n, tg, DEFERRED, 0.0)
        assert float(np.max(np.abs(w - dense)) / float(x[0])) <= MARGIN
    print('worst error of the dense solve %.3e, recorded %.3e' % (worst, DENSE_ERR))
