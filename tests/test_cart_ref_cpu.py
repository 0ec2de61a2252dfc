"""CPU: the extended-precision reference tests/cart_ref_ld.py pinned to the golden vectors, the float64 oracle
(oracle/adi_oracle.c) measured against it on every case of tests/cart_dt_cases.py, and the increment bar shown not to be vacuous.

1. The reference reproduces the Cartesian golden vectors to 1e-12 (it runs every step of a case in np.longdouble).
2. The oracle satisfies the bar of cart_dt_cases with A / 4 on every case; its worst distance from the reference at cfl <= 1e-3,
   in units of eps64 max|W|, is the figure A is taken from, and the recorded figure is held to the measured one.
3. Two mutants of the oracle are rejected by the bar: a time step 1 % off (every case with cfl >= 1e-11) and the identity
   (every case).  At cfl <= 1e-9 the first passes rel_linf <= 1e-10, the metric of the other parity tests: the gap, pinned.
Measured figures: DESIGN.md, "What the oracle is itself measured against"."""
import functools

import numpy as np
import pytest

import cart_dt_cases as cd
import cart_ref_ld
import cases
from helpers import golden, rel_linf, run_cart_case
from oracle import adi_oracle


@pytest.mark.parametrize('name', ['kat2', 'holes_mixed', 'long_line_70', 'edge_shapes'])
def test_long_double_reference_reproduces_the_golden_vectors(name):
    """kat2: Dirichlet plane, flux and per-face h on a disk; holes_mixed: 30 % holes, every kind of boundary data as arrays and
    scalars, theta = 1; long_line_70: ragged long lines; edge_shapes: a unit axis, an isolated cell, empty lines"""
    g = golden('cart', name)
    out = run_cart_case(cart_ref_ld, cases.cart_case(name))
    for key in ('T_step1', 'T_final'):
        assert out[key].dtype == np.longdouble
        err = rel_linf(out[key].astype(np.float64), g[key])
        assert err <= 1e-12, (name, key, err)


@functools.lru_cache(maxsize=None)
def _measured(key):
    """the oracle, the oracle with dt * 1.01 and the identity against the long-double reference: figures only"""
    c = cd.case(key)
    X = run_cart_case(adi_oracle, c)['T_final']
    Xa = run_cart_case(adi_oracle, cd.case(key, dt_factor=1.01))['T_final']
    return dict(oracle=cd.figures(X, key), finite=bool(np.all(np.isfinite(X))), exact=cd.untouched_cells_are_exact(X, key),
                dt_off=cd.figures(Xa, key), dt_off_old_metric=rel_linf(Xa, X), identity=cd.figures(np.array(c['T0']), key))


@pytest.mark.parametrize(**cd.params())
def test_oracle_within_a_quarter_of_the_bar_of_the_long_double_reference(key):
    m = _measured(key)
    f = m['oracle']
    print('oracle vs long double: %-72s inc %.2e K  err %.2e K = %6.2f ulp = %.1e inc' % (cd.tag(key), f['inc'], f['abs_err'],
                                                                                         f['ulp'], f['of_inc']))
    assert m['finite'] and m['exact']
    assert f['abs_err'] <= cd.bar(f, cd.A / 4), (cd.tag(key), f)


def test_recorded_oracle_worst_is_the_measured_one():
    """ORACLE_WORST_ULP is not below the measured worst and not above twice it, and A is 4 times it, rounded up to 2^n"""
    worst = max(_measured(k)['oracle']['ulp'] for k in cd.keys() if k[-1] <= 1e-3)
    print('worst oracle error at cfl <= 1e-3: %.3f eps64 max|W|; recorded %.3f, A = %g' % (worst, cd.ORACLE_WORST_ULP, cd.A))
    assert worst <= cd.ORACLE_WORST_ULP <= 2.0 * worst, (worst, cd.ORACLE_WORST_ULP)
    assert cd.A == cd.bar_factor(cd.ORACLE_WORST_ULP)


@pytest.mark.parametrize(**cd.params(lambda key: key[-1] >= 1e-11))
def test_bar_rejects_a_time_step_one_percent_off(key):
    f = _measured(key)['dt_off']
    assert f['abs_err'] > cd.bar(f, cd.A), (cd.tag(key), f)


@pytest.mark.parametrize(**cd.params())
def test_bar_rejects_the_identity(key):
    f = _measured(key)['identity']
    assert f['abs_err'] > cd.bar(f, cd.A), (cd.tag(key), f)


def test_switch_pairs_lie_either_side_of_the_gate_of_the_kernels():
    """theta*gamma of the third and fourth time step of every theta straddle kMixedMinTg as csrc/adi_core.hpp has it"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'adi_thermal_fields_amd', 'csrc',
                            'adi_core.hpp')).read()
    gate = float(re.search(r'constexpr double kMixedMinTg = ([0-9.eE+-]+);', src).group(1))
    assert gate == cd.K_MIXED_MIN_TG
    for theta, cfls in cd.CFL.items():
        assert theta * cfls[2] < gate < theta * cfls[3] and cfls[3] / cfls[2] < 1.2, (theta, cfls[2:4])


def test_field_relative_metric_accepts_the_one_percent_mutant_at_tiny_time_steps():
    """the gap the increment bar closes: with cfl <= 1e-9 a step with dt 1 % off is within 1e-10 of the field of the oracle"""
    ks = [k for k in cd.keys() if k[-1] <= 1e-9]
    assert {k[-1] for k in ks} == {1e-13, 1e-11, 0.95e-9}
    for k in ks:
        m = _measured(k)
        assert m['dt_off_old_metric'] <= 1e-10, (cd.tag(k), m['dt_off_old_metric'])
        assert m['dt_off']['of_inc'] > 5e-3, (cd.tag(k), m['dt_off'])       # ... while it is ~1 % of the step's change off
