"""GPU: the slab-decomposed step's increment against the extended-precision reference tests/cart_ref_ld.py, gamma = alpha dt/dx^2
from 1e-13 to 1e6, one step per case (tests/slab_dt_cases.py: grids, option sets, runner, expected forms; tests/cart_dt_cases.py:
metric, bar and why rel_linf cannot see these regimes).  dist_slab.SlabStepper over slab_engine.HipEngine, the ranks as threads
of one process on one GPU (dist_slab.LocalComm), at the shapes of slab_dt_cases.GRIDS.

Every case: finite; off-mask cells bit-equal to T0 and Dirichlet cells to dir_value;
    max over in-mask cells |HIP - W|  <=  A eps64 max|W| + 1e-10 max|W - T0|,
A = cart_dt_cases.A (taken from the float64 oracle's distance from W, not from the kernels); and the form of the sharded-axis
sweep the case is pinned to.  The pinned forms cover all six forms on both sides of theta*gamma = kMixedMinTg and at theta 0.5 and
1.  Then: an event loop's sequence of time steps under the quick planner (holes, curved), and a second step behind a prefetched
halo.  Next to each figure of the slab step the oracle's and the single-domain HIP step's are printed; the printout is
profiles/slab_increment_figures.txt, its worst figures per form are in DESIGN.md."""
import functools

import pytest

import slab_dt_cases as sd
from helpers import run_cart_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


def _report(what, tag, f):
    print('%-7s %-58s inc %.2e K  err %.2e K = %8.2f ulp = %.1e inc' % (what, tag, f['inc'], f['abs_err'], f['ulp'], f['of_inc']))


@functools.lru_cache(maxsize=None)
def _one_domain(grid, theta, cfl):
    """figures of the oracle and of the single-domain HIP step, once per (grid, theta, cfl)"""
    from oracle import adi_oracle
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    key = (grid, None, theta, cfl)
    c = sd.case(key, True)
    return tuple(sd.figures(run_cart_case(api, c)['T_final'], key, True) for api in (adi_oracle, hip))


@pytest.mark.parametrize(**sd.params())
def test_one_step_vs_long_double_reference(hip, key):
    grid, opt, theta, cfl = key
    tag = sd.tag(key)
    for what, f in zip(('oracle', 'hip-one'), _one_domain(grid, theta, cfl)):
        _report(what, tag, f)
    run = sd.run_case(sd.hip_engine, hip, key, True)
    f = sd.figures(run.T, key, True)
    (mode, fused, dots, quick), = run.plans[-1]                 # every rank under the same plan
    _report('slabs', '%s %s%s' % (tag, mode, ' dots' if dots else ' fused' if fused else ''), f)
    sd.hold(run.T, sd.case(key, True), f, tag)
    assert mode == sd.expected_form(key, True) and not quick, (tag, mode)


def test_pinned_forms_cover_every_form_either_side_of_the_gate_and_both_thetas():
    sd.forms_cover(True)


@pytest.mark.parametrize('grid', ['holes', 'curved'])
def test_quick_plans_over_a_sequence_of_time_steps_that_hops_regimes(hip, grid):
    sd.sequence_holds(sd.hip_engine, hip, grid, True)


_SECOND = [(g, o, cfl) for g in ('holes', 'solid') for o in sd.GRID_OPTS[g] for cfl in (2.1e-9, 1e6)]


@pytest.mark.parametrize('grid,opt,cfl', _SECOND, ids=['%s-%s-cfl%g' % t for t in _SECOND])
def test_second_step_behind_a_prefetched_halo(hip, grid, opt, cfl):
    """just above theta*gamma = kMixedMinTg and at the largest gamma: step 1 with prefetch_halo=True (the boundary planes of its
    result computed first and sent ahead), step 2 on the state as it stays on the device, judged from step 1's downloaded result"""
    key = (grid, opt, 0.5, cfl)
    c = sd.case(key, True)
    run = sd.run_slabs(sd.hip_engine, hip, c, sd.sizes(key), dict(sd.options(key, True), prefetch=True), nsteps=2, keep_steps=True)
    f1 = sd.figures(run.steps[0], key, True)
    sd.hold(run.steps[0], c, f1, (sd.tag(key), 1))
    f2, c2 = sd.step_figures(run.steps[1], c, run.steps[0], c['dt'])
    _report('step 2', '%s %s' % (sd.tag(key), '/'.join(sorted(run.modes))), f2)
    sd.hold(run.steps[1], c2, f2, (sd.tag(key), 2))
