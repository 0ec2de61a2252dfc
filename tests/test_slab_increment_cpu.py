"""CPU: the slab-decomposed step's increment against the extended-precision reference tests/cart_ref_ld.py, gamma = alpha dt/dx^2
from 1e-13 to 1e6, one step per case (tests/slab_dt_cases.py: grids, option sets, runner, expected forms).  dist_slab.SlabStepper
with the reference engine tests/cpu_engine.py, ranks as threads over LocalComm, the slabs and nx of the GPU test on small planes:
the planner, the exchange and the algebra of every form of the sharded-axis sweep, without a GPU.

1. Every case: finite, off-mask cells bit-equal to T0 and Dirichlet cells to dir_value, and the bar of cart_dt_cases,
       max over in-mask cells |X - W|  <=  A eps64 max|W| + 1e-10 max|W - T0|,
   in the form the case is pinned to (slab_dt_cases.FORMS_CPU).
2. The pinned forms cover all six forms, on both sides of theta*gamma = kMixedMinTg and at theta 0.5 and 1.
3. Mutants the field-relative metric of the other slab tests accepts and the bar rejects: ranks that do not talk to each other
   (interface values zeroed), and deferred weights built for a time step 1 % off.
4. An event loop's sequence of time steps under the quick planner, every step judged from its own input."""
import pytest

import cart_dt_cases as cd
import slab_dt_cases as sd
from cpu_engine import CpuEngine
from oracle import adi_oracle as orc


@pytest.mark.parametrize(**sd.params())
def test_one_step_vs_long_double_reference(key):
    run = sd.run_case(CpuEngine, orc, key, False)
    f = sd.figures(run.T, key, False)
    (mode, fused, dots, quick), = run.plans[-1]                 # every rank under the same plan
    print('cpu %-46s %-15s inc %.2e K  err %.2e K = %8.2f ulp = %.1e inc' % (sd.tag(key), mode, f['inc'], f['abs_err'], f['ulp'],
                                                                              f['of_inc']))
    sd.hold(run.T, sd.case(key, False), f, sd.tag(key))
    assert mode == sd.expected_form(key, False) and not quick, (sd.tag(key), mode)


def test_pinned_forms_cover_every_form_either_side_of_the_gate_and_both_thetas():
    sd.forms_cover(False)


# ---- 3. mutants ------------------------------------------------------------------------------------------------------------
class _SilentRanks(CpuEngine):
    """interface values zeroed: no coupling between the slabs at all"""

    def interface_pair(self, my_lo, my_hi, prev_hi, next_lo, nlines, xlo, xhi):
        xlo.zero_(); xhi.zero_()

    def interface(self, cond_all, world, rank, nlines, xlo, xhi):
        xlo.zero_(); xhi.zero_()

    def interface_deferred(self, first, last, prev_last, next_first, omega, nlines, ulo, uhi):
        ulo.zero_(); uhi.zero_()


class _WeightsOnePercentOff(CpuEngine):
    """the deferred form's weights built for a time step 1 % off"""

    def deferred_setup(self, n, theta, gam, tol):
        return CpuEngine.deferred_setup(self, n, theta, 1.01 * gam, tol)


@pytest.mark.parametrize('grid,form', [('holes', 'window'), ('solid', 'deferred')])
@pytest.mark.parametrize('cfl,old_bar', [(1e-13, 1e-13), (1e-11, 1e-10)])
def test_bar_rejects_ranks_that_do_not_talk(grid, form, cfl, old_bar):
    """... which the strictest field-relative bar of the slab tests (1e-13) accepts at cfl 1e-13, and their 1e-10 at cfl 1e-11"""
    key = (grid, 'default', 0.5, cfl)
    run = sd.run_case(_SilentRanks, orc, key, False)
    assert run.modes == {form}
    f = sd.figures(run.T, key, False)
    print('silent ranks %s: rel_linf %.2e, abs_err / bar = %.1f' % (sd.tag(key), f['abs_err'] / f['wmax'], f['abs_err'] / cd.bar(f, sd.A)))
    assert f['abs_err'] / f['wmax'] <= old_bar, f
    assert f['abs_err'] > 4.0 * cd.bar(f, sd.A), f


@pytest.mark.parametrize('grid', ['solid', 'thin_solid'])
def test_bar_rejects_deferred_weights_of_a_time_step_one_percent_off(grid):
    """cfl 1e-11 (picked by running it): the correction is 1 % off -- 5e-14 of the field, 7 x the bar; at cfl 1e-13 it is below the
    rounding floor of a float64 field and no metric can see it"""
    key = (grid, 'default', 0.5, 1e-11)
    run = sd.run_case(_WeightsOnePercentOff, orc, key, False)
    assert run.modes == {'deferred'}
    f = sd.figures(run.T, key, False)
    print('weights 1 %% off %s: rel_linf %.2e, abs_err / bar = %.1f' % (sd.tag(key), f['abs_err'] / f['wmax'], f['abs_err'] / cd.bar(f, sd.A)))
    assert f['abs_err'] / f['wmax'] <= 1e-10, f
    assert f['abs_err'] > 4.0 * cd.bar(f, sd.A), f


# ---- 4. quick plans --------------------------------------------------------------------------------------------------------
def test_quick_plans_over_a_sequence_of_time_steps_that_hops_regimes():
    sd.sequence_holds(CpuEngine, orc, 'holes', False)
