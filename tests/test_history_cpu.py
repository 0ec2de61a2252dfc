"""CPU: the definition of the thermal-history recorder (ThermalHistory.record_reference / seed_reference, HistoryLevels) over the
pinned C oracle -- the conditions the cases of tests/history_cases.py were built for, the peak as a running maximum, exact
crossing fractions, the seeding rules, the argument rules of the C ABI, and the cooling time of a lumped body against its
closed form."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import history_cases as hc  # noqa: E402


@pytest.fixture(scope='module')
def mods():
    from adi_thermal_fields_amd.adi3d_hip_coeff import HistoryLevels, ThermalHistory
    from oracle import adi_oracle as orc
    return ThermalHistory, HistoryLevels, orc


_runs = {}


def _run(mods, name):
    """trajectory and recorded states of a case over the oracle, computed once"""
    TH, HL, orc = mods
    if name not in _runs:
        c = hc.case(name)
        traj = hc.oracle_trajectory(orc, c)
        _runs[name] = (c, traj) + hc.record_trajectory(TH, HL(*hc.LEVELS), c, traj)
    return _runs[name]


def test_levels_are_validated(mods):
    _, HL, _ = mods
    lv = HL(800.0, 500.0, 1400.0)
    assert lv.key() == (800.0, 500.0, 1400.0)
    c = lv.as_c()
    assert (c.T_hi, c.T_lo, c.T_melt) == (800.0, 500.0, 1400.0)
    assert HL(800.0, 500.0, 100.0).key()[2] == 100.0                  # T_melt is independent of the other two
    for bad in ((500.0, 500.0, 1.0), (400.0, 500.0, 1.0), (float('nan'), 1.0, 1.0), (2.0, 1.0, float('inf')), ('a', 1.0, 1.0)):
        with pytest.raises(ValueError):
            HL(*bad)


@pytest.mark.parametrize('name', hc.CASES)
def test_case_conditions(mods, name):
    """the inputs produce every kind of cell and of pool the device tests rely on"""
    c, traj, states, pools, times, t_end = _run(mods, name)
    assert 40 <= hc.nsteps(c) <= 60 and len({dt for dt, _, _ in c['segments']}) == 2
    got = hc.conditions(c, traj, states, pools)
    print(name, got)
    assert got['hi_only'] > 0 and got['cycle'] > 0 and got['both'] > 0 and got['reheated'] > 0, got
    assert got['pool_wide_step'] is not None and got['pool_empty_step'] is not None, got
    assert got['pool_empty_step'] > got['pool_wide_step']
    assert times[-1] == t_end and np.all(np.diff(times) > 0)


@pytest.mark.parametrize('name', hc.CASES)
def test_peak_is_the_running_maximum_and_off_mask_stays_nan(mods, name):
    c, traj, states, pools, _, _ = _run(mods, name)
    mask = c['mask']
    run_max = np.array(traj[0])
    for n in range(1, len(traj)):
        run_max = np.maximum(run_max, traj[n])
        peak, t_hi, t_lo = states[n]
        assert np.array_equal(peak[mask], run_max[mask]), n
        assert np.all(peak[mask] >= traj[n][mask])
        for a in (peak, t_hi, t_lo):
            assert np.isnan(a[~mask]).all()
        # a recorded time lies inside the step that recorded it, and a cooling time is positive
        done = ~np.isnan(t_hi) & ~np.isnan(t_lo)
        assert np.all(t_lo[done] >= t_hi[done])
    # the precondition of the kernel's skip rule holds along the whole run: every A has been recorded
    for n in range(1, len(traj)):
        assert np.all(traj[n - 1][mask] <= states[n - 1][0][mask])


def test_exact_crossing_fractions(mods):
    TH, HL, _ = mods
    lv = HL(800.0, 500.0, 1400.0)
    #             hi only      lo only      both         none (rising)  touches T_hi from above   starts on T_hi
    A = np.array([[[900.0,      700.0,       1000.0,      400.0,         900.0,                    800.0]]])
    B = np.array([[[700.0,      300.0,       200.0,       900.0,         800.0,                    700.0]]])
    mask = np.ones(A.shape, dtype=bool)
    state = TH.seed_reference(hc.empty_state(A.shape), A, mask)
    # a stale t_lo everywhere: rule 2 must clear it, nothing else may touch it
    state = (state[0], state[1], np.full(A.shape, -7.0))
    t_n, dt = 3.0, 0.25
    (peak, t_hi, t_lo), pool = TH.record_reference(state, A, B, mask, t_n, dt, lv)
    assert t_hi[0, 0, 0] == t_n + 0.5 * dt and np.isnan(t_lo[0, 0, 0])
    assert np.isnan(t_hi[0, 0, 1]) and t_lo[0, 0, 1] == t_n + 0.5 * dt
    assert t_hi[0, 0, 2] == t_n + 0.25 * dt and t_lo[0, 0, 2] == t_n + 0.625 * dt
    assert np.isnan(t_hi[0, 0, 3]) and t_lo[0, 0, 3] == -7.0 and peak[0, 0, 3] == 900.0
    assert t_hi[0, 0, 4] == t_n + dt and np.isnan(t_lo[0, 0, 4])       # B <= T_hi counts as crossed, at the end of the step
    assert np.isnan(t_hi[0, 0, 5]) and t_lo[0, 0, 5] == -7.0           # A > T_hi is strict: no crossing from T_hi itself
    assert np.array_equal(peak, np.maximum(A, B))
    assert pool['cells'] == 0 and list(pool['lo']) == [2 ** 31 - 1] * 3 and list(pool['hi']) == [-1] * 3
    # the pool counts B >= T_melt, the level included, on the mask only
    B2 = np.array([[[1400.0, 1399.0, 1500.0, 1400.0, 0.0, 2000.0]]])
    m2 = mask.copy()
    m2[0, 0, 5] = False
    _, pool = TH.record_reference(state, A, B2, m2, t_n, dt, lv)
    assert pool['cells'] == 3 and list(pool['lo']) == [0, 0, 0] and list(pool['hi']) == [0, 0, 3]


def test_a_peak_on_t_lo_holds_no_crossing(mods):
    """the kernel looks for crossings only in bricks with an old peak ABOVE T_lo; a brick whose peak equals T_lo exactly has
    A <= T_lo everywhere (the precondition), and A > T_lo is strict, so the definition records nothing there either"""
    TH, HL, _ = mods
    lv = HL(800.0, 500.0, 1400.0)
    shape = (3, 3, 3)
    A, B = np.full(shape, 500.0), np.full(shape, 300.0)
    mask = np.ones(shape, dtype=bool)
    state = TH.seed_reference(hc.empty_state(shape), A, mask)
    (peak, t_hi, t_lo), _ = TH.record_reference(state, A, B, mask, 0.0, 1.0, lv)
    assert np.array_equal(peak, A) and np.isnan(t_hi).all() and np.isnan(t_lo).all()


def test_seed_and_sync_mask_semantics(mods):
    TH, _, _ = mods
    rng = np.random.default_rng(3)
    shape = (4, 5, 6)
    old = rng.random(shape) > 0.4
    state = tuple(np.where(old, rng.random(shape) + i, np.nan) for i in range(3))
    new = old.copy()
    born, gone = np.argwhere(~old)[::2], np.argwhere(old)[::3]
    new[tuple(born.T)] = True
    new[tuple(gone.T)] = False
    T = rng.random(shape) + 10.0
    sel = new & ~old                                     # what ThermalHistory.sync_mask selects: the newborn cells
    peak, t_hi, t_lo = TH.seed_reference(state, T, new, sel)
    keep = new & old
    for got, was in zip((peak, t_hi, t_lo), state):
        assert np.array_equal(got[keep], was[keep])      # every other in-mask cell keeps its state
        assert np.isnan(got[~new]).all()                 # cells that left the mask (and those never in it) are NaN
    assert np.array_equal(peak[sel], T[sel]) and np.isnan(t_hi[sel]).all() and np.isnan(t_lo[sel]).all()
    assert len(born) and len(gone)
    # without a selection every in-mask cell is seeded
    peak, t_hi, t_lo = TH.seed_reference(state, T, new)
    assert np.array_equal(peak[new], T[new]) and np.isnan(t_hi).all() and np.isnan(t_lo).all()


def test_argument_errors_without_gpu():
    """every rule is checked before any HIP call"""
    from adi_thermal_fields_amd import _lib
    lib, P = _lib.lib, ctypes.c_void_p
    assert _lib.HISTORY_BLOCK_BYTES == 40 and _lib.HISTORY_LOG_INTS == 8
    lv = _lib.HistoryLevelsC(800.0, 500.0, 1400.0)
    ok = [ctypes.byref(lv), P(8), P(16), P(24), P(32), P(40), P(48), P(56), P(64), None, 4, 4, 4, 0, None]

    def rec(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.adi_history_record(*a)
    for i in range(9):
        with pytest.raises(ValueError, match='null argument'):
            _lib.check(rec(**{'a%d' % i: None}))
    with pytest.raises(ValueError, match='aliases d_T_in'):
        _lib.check(rec(a3=P(16)))
    for i in (4, 5, 6):
        for j in (2, 3):
            with pytest.raises(ValueError, match='a state array aliases T'):
                _lib.check(rec(**{'a%d' % i: ok[j]}))
    with pytest.raises(ValueError, match='state arrays alias'):
        _lib.check(rec(a5=P(32)))
    for bad in ((float('nan'), 500.0, 1.0), (800.0, float('inf'), 1.0), (800.0, 500.0, float('nan'))):
        with pytest.raises(ValueError, match='not finite'):
            _lib.check(rec(a0=ctypes.byref(_lib.HistoryLevelsC(*bad))))
    for bad in ((500.0, 500.0, 1.0), (400.0, 500.0, 1.0)):
        with pytest.raises(ValueError, match='T_hi must be above T_lo'):
            _lib.check(rec(a0=ctypes.byref(_lib.HistoryLevelsC(*bad))))
    with pytest.raises(ValueError, match='bad grid'):
        _lib.check(rec(a10=0))
    with pytest.raises(ValueError, match='too large'):
        _lib.check(rec(a10=16 * 65536, a11=1, a12=1))
    with pytest.raises(ValueError, match='capacity'):
        _lib.check(lib.adi_history_reset_log(P(8), P(16), 0, None))
    with pytest.raises(ValueError, match='null'):
        _lib.check(lib.adi_history_reset_log(None, P(16), 4, None))
    with pytest.raises(ValueError, match='null'):
        _lib.check(lib.adi_history_tick(None, None))
    with pytest.raises(ValueError, match='null'):
        _lib.check(lib.adi_history_set_clock(None, 0.0, 1.0, None))
    for t0, dt in ((float('nan'), 1.0), (0.0, 0.0), (0.0, float('inf'))):
        with pytest.raises(ValueError, match='bad t0 / dt'):
            _lib.check(lib.adi_history_set_clock(P(8), t0, dt, None))
    seed_ok = [P(8), P(16), P(24), P(32), P(40), None, None, 4, 4, 4, 0, None]
    for i in range(5):
        a = list(seed_ok)
        a[i] = None
        with pytest.raises(ValueError, match='null argument'):
            _lib.check(lib.adi_history_seed(*a))
    a = list(seed_ok)
    a[2] = P(8)
    with pytest.raises(ValueError, match='aliases T'):
        _lib.check(lib.adi_history_seed(*a))
    a = list(seed_ok)
    a[3] = P(16)
    with pytest.raises(ValueError, match='state arrays alias'):
        _lib.check(lib.adi_history_seed(*a))


def test_lumped_body_cooling_time(mods):
    """An 8^3 cube of 1 mm cells at 1000 degrees, Robin h = 200 W/m^2K on all six faces into 25 degrees (Biot number
    h (a/6) / k = 0.005): every cell's t8/5 from the definition over the C oracle (dt = 0.1 s) against the lumped body's
    tau ln((800 - Tinf)/(500 - Tinf)), tau = rho cp a / (6 h) = 25.48 s, which is 12.4737 s.
    Measured here: every cell gives 12.5223 s, 0.0486 s (0.39 %) above the closed form: the body is not exactly lumped (its
    surface runs colder than its centre, so it loses a little less than the lumped body does) and the crossings are interpolated
    linearly.  The bar is twice the measured error, 0.0972 s, which is tighter than one dt."""
    TH, HL, orc = mods
    n, dx, h, Tinf, T0, dt = 8, 1e-3, 200.0, 25.0, 1000.0, 0.1
    a = n * dx
    tau = hc.RHO * hc.CP * a / (6.0 * h)
    want = tau * math.log((800.0 - Tinf) / (500.0 - Tinf))
    measured = 0.0486
    bar = min(2.0 * measured, dt)
    lv = HL(800.0, 500.0, 1400.0)
    mask = np.ones((n, n, n), dtype=bool)
    grid, mat, prm = orc.Grid3D(n, n, n, dx, mask), orc.Material(hc.RHO, hc.CP, hc.K), orc.Params(dt, 0.5)
    packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h={f: h for f in hc.FACES})
    T = np.full(mask.shape, T0)
    state = TH.seed_reference(hc.empty_state(mask.shape), T, mask)
    nst = int(math.ceil(1.2 * tau * math.log((T0 - Tinf) / (500.0 - Tinf)) / dt))
    for i in range(nst):
        Tn = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
        state, pool = TH.record_reference(state, T, Tn, mask, 0.0 + i * dt, dt, lv)
        assert pool['cells'] == 0
        T = Tn
    t85 = state[2] - state[1]
    assert not np.isnan(t85).any()
    err = float(np.abs(t85 - want).max())
    print('lumped body: t8/5 analytic %.4f s, cells %.4f .. %.4f s, max error %.4f s (bar %.4f s, dt %.3f s)'
          % (want, t85.min(), t85.max(), err, bar, dt))
    assert err <= bar
