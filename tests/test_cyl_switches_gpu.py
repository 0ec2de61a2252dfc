"""GPU: the cylindrical step at every kernel switch, in place, and over the range of time steps.

1. One deterministic case per dispatch decision of csrc/adi_cyl.hip (cyl_switch_cases.SWITCH_CASES: the id of a test names
   the kernel it is meant to reach; profiles/cyl_switches_kernel_trace.txt is the kernel trace of this file), plain, with a
   source field and masked, on a full cylinder and on an annulus, against oracle/cyl_oracle.py at BASELINE.json's 1e-10.
2. The sweeps in place: adi_cyl_sweep allows d_out == d_in because every thread reads only the rows it later writes.  Out
   of place and in place are the same kernels on the same values, so any difference between adi_step, StagedCylStepper.step
   (phi and z in place) and StagedCylStepper.run (all three in place) is a read-after-write hazard.
3. alpha*dt/dr^2 from 1e-13 to 1e6 against the extended-precision reference tests/cyl_ref_ld.py (the float64 oracle is held
   to a tenth of the bar against the same reference by tests/test_cyl_ref_cpu.py), at 1e-10 of the field and, since that
   bar passes anything at f <= 1e-9, at the increment bar of tests/cart_dt_cases.py: A_CYL eps64 max|W| + 1e-10 max|W - T0|.
Measured figures: DESIGN.md, "Cylindrical kernels: what reaches what"."""
import numpy as np
import pytest

import cart_dt_cases as cd
import cyl_switch_cases as csc
from helpers import rel_linf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hipcyl():
    import adi_thermal_fields_amd.adi3d_hip_cyl as m
    return m


# ---- 1. every dispatch decision -------------------------------------------------------------------------------------------
_SWITCH = csc.switch_params()


@pytest.mark.parametrize('tag,spec', _SWITCH, ids=[t for t, _ in _SWITCH])
def test_switch_case_vs_oracle(hipcyl, tag, spec):
    from oracle import cyl_oracle
    c = csc.make_case(**spec)
    got = csc.run_case(hipcyl, c)
    want = csc.run_case(cyl_oracle, c)
    err = rel_linf(got, want)
    print('switch %-72s %.3e' % (tag, err))
    assert np.all(np.isfinite(got))
    assert err <= 1e-10, (tag, err)
    if c['active'] is not None:
        act = c['active']
        # void cells hold robin_void.T_inf, inactive cells of the axis row robin_inner.T_inf: written, not computed
        assert np.array_equal(got[1:][~act[1:]], np.full(int((~act[1:]).sum()), csc.ROBIN_VOID[1]))
        assert np.array_equal(got[0][~act[0]], np.full(int((~act[0]).sum()), csc.ROBIN_INNER[1]))
        assert np.array_equal(got[~act], want[~act])


@pytest.mark.parametrize('shape', [(1025, 2, 3), (2, 1025, 3), (2, 3, 1025)], ids=['nr1025', 'nphi1025', 'nz1025'])
def test_axis_longer_than_1024_is_refused_before_any_launch(hipcyl, shape):
    """argument validation of the plan: it returns before any launch, and the next valid step is served as usual"""
    from oracle import cyl_oracle
    c = csc.make_case(shape)
    with pytest.raises(ValueError, match='axis longer than 1024 cells is not supported'):
        csc.run_case(hipcyl, c)
    ok = csc.make_case((17, 3, 5))
    assert rel_linf(csc.run_case(hipcyl, ok), csc.run_case(cyl_oracle, ok)) <= 1e-10


# ---- 2. in place ----------------------------------------------------------------------------------------------------------
INPLACE = [('r_fast16', (256, 8, 16)), ('r_fast8', (64, 16, 4)),
           ('r_strided8', (512, 3, 5)), ('r_strided16', (1024, 2, 9)),
           ('phi_strided8', (3, 192, 32)), ('phi_strided16', (2, 1024, 8)),
           ('phi_fast8', (3, 64, 32)), ('phi_fast16_Lp32', (2, 512, 32)),
           ('z_fast_lwf1', (3, 3, 1024)), ('z_fast_lwf8', (3, 8, 128)),
           ('z_contig4', (3, 5, 256)), ('z_contig8', (3, 5, 512)), ('z_contig16_scalar', (2, 3, 1000)),
           ('z_contig16_vec', (2, 3, 768))]
GRAPHED = ('r_fast16', 'phi_fast16_Lp32')       # the graph replay at two shapes only: capture cost stays out of the others


@pytest.mark.parametrize('name,shape', INPLACE, ids=['%s-%dx%dx%d' % ((n,) + s) for n, s in INPLACE])
def test_in_place_sweeps_are_bit_identical_to_out_of_place(hipcyl, name, shape):
    c = csc.make_case(shape, nsteps=5)
    grid, mat, prm, rr, zbc = csc.api_objects(hipcyl, c)
    a = hipcyl.to_device(c['T0'])
    for _ in range(5):
        a = hipcyl.adi_step(a, grid, mat, prm, rr, zbc)             # (a) a fresh output every step
    a = a.get()
    assert np.all(np.isfinite(a))
    st = hipcyl.StagedCylStepper(grid, mat, prm, rr, zbc)
    b = hipcyl.to_device(c['T0'])
    for _ in range(5):
        b = st.step(b)                                              # (b) r out of place, phi and z in place
    assert np.array_equal(b.get(), a)
    assert np.array_equal(st.run(hipcyl.to_device(c['T0']), 5, graph=False).get(), a)      # (c) all three in place
    if name in GRAPHED:
        assert np.array_equal(st.run(hipcyl.to_device(c['T0']), 5, graph=True).get(), a)   # (d) captured, replayed ...
        assert np.array_equal(st.run(hipcyl.to_device(c['T0']), 5, graph=True).get(), a)   # ... and replayed again


# ---- 3. the range of time steps ---------------------------------------------------------------------------------------------
_DT = csc.dt_params()


@pytest.mark.parametrize('tag,key', _DT, ids=[t for t, _ in _DT])
def test_time_step_range_vs_long_double_reference(hipcyl, tag, key):
    """alpha*dt/dr^2 = 1e-13 ... 1e6, Robin closures on r and both z ends, two steps.  At R_in = 0 the phi factor
    alpha*dt/(r^2 dphi^2) of the first radius off the axis is (nphi / 3 pi)^2 times larger: 2.95e9 at nphi = 512, f = 1e6.
    Measured on the MI355X, worst over the shapes per f: 1.3e-15, 1.5e-15, 1.9e-15, 2.1e-14, 3.8e-11, 2.4e-11 -- the last two
    at (2, 512, 32) on the axis, the cost of the Sherman-Morrison closure at phi factors of 8.9e7 and 2.95e9."""
    _, want = csc.dt_reference(*key)
    got = csc.run_case(hipcyl, csc.dt_case(*key))
    err = rel_linf(got, want)
    print('dt range %-44s %.3e' % (tag, err))
    assert np.all(np.isfinite(got))
    assert err <= 1e-10, (tag, err)
    # the same result against what the two steps changed (cart_dt_cases: metric and bar; A_CYL from the oracle, on the CPU).
    # The (2, 512, 32) axis cases above are ~4e-8 K off where the two steps moved the field by ~1e3 K: within 1e-10 of that.
    f = cd.cyl_figures(got, key)
    print('         %-44s inc %.2e K  err %.2e K = %8.2f ulp = %.1e inc' % ('', f['inc'], f['abs_err'], f['ulp'], f['of_inc']))
    assert f['abs_err'] <= cd.bar(f, cd.A_CYL), (tag, f, cd.bar(f, cd.A_CYL))
