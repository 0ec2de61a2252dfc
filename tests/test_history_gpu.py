"""GPU: the thermal-history recorder on the device -- adi_history_record / adi_history_seed through ThermalHistory, the `history=`
argument of adi_step_numba_coeff / StagedStepper and of the waam loops -- against the definition, ThermalHistory.record_reference,
fed with the fields of the same run without a recorder.

Bars: T_peak, t_hi, t_lo np.array_equal with NaN in the same places, the log rows equal as integers (IEEE subtract / divide /
multiply / add in one fixed order on both sides, contraction off; integer atomics); the T trajectory with the recorder
bit-identical to the one without; graph replay against the same launches issued one by one: bit-identical."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import history_cases as hc  # noqa: E402
from history_cases import CP, K, KAPPA, RHO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


VARIANTS = [('holes', None), ('holes', hc.PADDED['holes']), ('solid', None)]
IDS = ['holes', 'holes_padded', 'solid']


def _pad(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _state(h):
    return np.asarray(h.T_peak), np.asarray(h.t_hi), np.asarray(h.t_lo)


def _assert_state(h, want, what):
    for name, got, w in zip(('T_peak', 't_hi', 't_lo'), _state(h), want):
        assert _same(got, w), (what, name, int((~((got == w) | (np.isnan(got) & np.isnan(w)))).sum()))


def _log_rows(h, n):
    return h.d_log.cpu().numpy().reshape(h.capacity + 1, 8)[:n]


def _guards_intact(h):
    g = h._log_store.cpu().numpy()
    return bool((g[:h.LOG_GUARD] == h.GUARD_WORD).all() and (g[-h.LOG_GUARD:] == h.GUARD_WORD).all())


def _trajectory(hip, c, grid, mat, packs, history=None, on_step=None):
    """the case with single launches, every field downloaded; the source segment in its field form"""
    T = hip.to_device(np.array(c['T0']))
    traj = [np.asarray(T)]
    for dt, n, S in c['segments']:
        prm = hip.Params(dt, hc.THETA)
        d_S = None if S is None else hip.to_device(np.array(S))
        for _ in range(n):
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=hc.TINF, S=d_S, history=history)
            traj.append(np.asarray(T))
            if on_step is not None:
                on_step(len(traj) - 1)
    return traj


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_kernel_against_the_definition(mods, monkeypatch, name, phys):
    hip = mods
    _pad(monkeypatch, hip, phys)
    c = hc.case(name)
    grid, mat, packs = hc.setup(hip, c)
    if phys is not None:
        assert grid.layout.padded and grid.layout.pd[:3] == phys
    if name == 'solid':
        assert grid.all_solid                                     # the flags summary says all-solid: no flags are loaded
    lv = hip.HistoryLevels(*hc.LEVELS)
    plain = _trajectory(hip, c, grid, mat, packs)
    states, pools, times, t_end = hc.record_trajectory(hip.ThermalHistory, lv, c, plain, clock='step')
    got = hc.conditions(c, plain, states, pools)
    print(name, got)
    assert min(got['hi_only'], got['cycle'], got['both'], got['reheated']) > 0 and got['pool_empty_step'] is not None, got
    h = hip.ThermalHistory(grid, lv, capacity=hc.nsteps(c) + 3, T=hip.to_device(np.array(c['T0'])))
    _assert_state(h, states[0], 'seed')
    ptrs = h.graph_key()

    def on_step(n):
        _assert_state(h, states[n], 'step %d' % n)
    with_h = _trajectory(hip, c, grid, mat, packs, history=h, on_step=on_step)
    for n, (a, b) in enumerate(zip(plain, with_h)):
        assert np.array_equal(a, b), n                           # the recorder never touches T
    n = hc.nsteps(c)
    assert h.slot == n and h.t == t_end
    assert np.array_equal(_log_rows(h, n), hc.pool_rows(pools))
    mp = h.melt_pool()
    assert mp['dropped'] == 0 and np.array_equal(mp['t'], np.array(times)) and np.array_equal(mp['cells'], [p['cells'] for p in pools])
    k = got['pool_empty_step'] - 1
    assert mp['volume'][k] == 0.0 and not mp['extent'][k].any() and mp['extent'][0].min() > 0.0
    assert np.array_equal(mp['extent'][0], (mp['hi'][0] - mp['lo'][0] + 1) * hc.DX)
    ct = np.asarray(h.cooling_time)
    assert _same(ct, states[-1][2] - states[-1][1])
    assert ptrs == h.graph_key() and _guards_intact(h)


def test_graph_replay(mods):
    """StagedStepper.run through the graph against the same launches one by one: fields, log and clock bit-identical, and both
    equal to the definition over the stepper's own single steps; 7 steps of one dt (a graph of two steps and a tail step), then
    24 of another on the same recorder"""
    hip = mods
    c = hc.case('holes')
    grid, mat, packs = hc.setup(hip, c)
    lv = hip.HistoryLevels(*hc.LEVELS)
    segs = [(hc.DT_A, 7, None), (hc.DT_B, 24, None)]
    T0 = np.array(c['T0'])
    traj = [T0]
    T = hip.to_device(T0)
    for dt, n, _ in segs:
        st = hip.StagedStepper(grid, mat, hip.Params(dt, hc.THETA), packs, hc.TINF)
        for _ in range(n):
            T = st.step(T)
            traj.append(np.asarray(T))
    states, pools, times, t_end = hc.record_trajectory(hip.ThermalHistory, lv, c, traj, t=1.5, clock='run', segments=segs)
    h = hip.ThermalHistory(grid, lv, capacity=64, T=hip.to_device(T0), t=1.5)
    sa = hip.StagedStepper(grid, mat, hip.Params(hc.DT_A, hc.THETA), packs, hc.TINF, history=h)
    sb = hip.StagedStepper(grid, mat, hip.Params(hc.DT_B, hc.THETA), packs, hc.TINF, history=h)
    res = {}
    for how in ('graph', 'graph again', 'launches'):
        h.reset(hip.to_device(T0), t=1.5)
        T = sa.run(hip.to_device(T0), 7, graph=how != 'launches')
        assert h.slot == 7 and h.t == 1.5 + 7 * hc.DT_A
        _assert_state(h, states[7], how)
        T = sb.run(T, 24, graph=how != 'launches')                # another dt: the log and the clock go on
        res[how] = (np.asarray(T),) + _state(h) + (_log_rows(h, 31).copy(), h.t, h.melt_pool()['t'])
        assert h.slot == 31 and h.t == t_end
        _assert_state(h, states[31], how)
        assert np.array_equal(res[how][4], hc.pool_rows(pools))
        assert np.array_equal(res[how][6], np.array(times))
        assert np.array_equal(res[how][0], traj[-1])
    assert sa.captures == 1 and sb.captures == 1                  # the second run with the same key replays the first graph
    for how in ('graph again', 'launches'):
        for a, b in zip(res['graph'], res[how]):
            assert _same(a, b), how
    # other levels: another graph (they travel by value in the launch), and the new levels are the ones at work
    h.levels = hip.HistoryLevels(900.0, 450.0, 1400.0)
    h.reset(hip.to_device(T0), t=1.5)
    sa.run(hip.to_device(T0), 7)
    assert sa.captures == 2
    want, _, _, _ = hc.record_trajectory(hip.ThermalHistory, h.levels, c, traj[:8], t=1.5, clock='run', segments=segs[:1])
    _assert_state(h, want[7], 'new levels')
    assert not _same(want[7][1], states[7][1])
    assert _guards_intact(h)


def test_with_source_surface_loss_and_latent_heat(mods):
    """GoldakSource, LossPacks and PhaseField in one stepper on the 24 x 16 x 16 plate of tests/test_phase_gpu.py: B is the
    corrected field.  Single steps without a recorder give the fields; single steps and the graph with one must record what the
    definition makes of them, and leave T and f as they were"""
    hip = mods
    shape, dx = (24, 16, 16), 5e-4
    dt, theta, Tinf = 2.0 * dx * dx / KAPPA, 0.5, 25.0
    mask = np.ones(shape, dtype=bool)
    mask[:, :, 12:] = False
    mask[8:20, 6:10, 12:14] = True
    T0 = np.where(mask, 900.0, Tinf)
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    lv = hip.HistoryLevels(950.0, 920.0, 1450.0)                  # T_melt: the liquidus
    loss = hip.SurfaceLoss(h=15.0, emissivity=0.8)
    src = hip.GoldakSource(power=900.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                           origin=(7 * dx, 8 * dx, 14 * dx), velocity=0.02, travel_axis=0, travel_sign=1, depth_axis=2)
    nst = 8
    c = dict(shape=shape, mask=mask, segments=[(dt, nst, None)])
    grid, mat, prm = hip.Grid3D(*shape, dx, mask), hip.Material(RHO, CP, K), hip.Params(dt, theta)
    lp = hip.LossPacks(grid, mat, loss, Tinf)
    ph = hip.PhaseField(grid, mat, law, T=hip.to_device(T0))
    plain = hip.StagedStepper(grid, mat, prm, lp.packs, Tinf, source=src, surface_loss=lp, phase=ph)
    T = hip.to_device(T0)
    traj = [T0]
    for i in range(nst):
        T = plain.step(T, t=i * dt)
        traj.append(np.asarray(T))
    f_end = np.asarray(ph.liquid_fraction)
    assert f_end.max() == 1.0                                     # a pool: the correction is at work on B
    h = hip.ThermalHistory(grid, lv, capacity=nst, T=hip.to_device(T0))
    st = hip.StagedStepper(grid, mat, prm, lp.packs, Tinf, source=src, surface_loss=lp, phase=ph, history=h)
    for clock in ('step', 'run'):
        states, pools, times, t_end = hc.record_trajectory(hip.ThermalHistory, lv, c, traj, clock=clock)
        assert max(p['cells'] for p in pools) > 0 and np.isfinite(states[-1][1]).any()
        ph.seed(hip.to_device(T0))
        h.reset(hip.to_device(T0))
        T = hip.to_device(T0)
        if clock == 'step':
            for i in range(nst):
                T = st.step(T, t=i * dt)
                assert np.array_equal(np.asarray(T), traj[i + 1]), i
                _assert_state(h, states[i + 1], 'step %d' % (i + 1))
        else:
            T = st.run(T, nst, t0=0.0)
            assert np.array_equal(np.asarray(T), traj[-1])
        _assert_state(h, states[-1], clock)
        assert np.array_equal(np.asarray(ph.liquid_fraction), f_end)
        assert np.array_equal(_log_rows(h, nst), hc.pool_rows(pools)) and h.t == t_end and h.slot == nst
    assert st.captures == 1


def test_log_overflow(mods):
    """capacity 3, 5 steps: three rows, two steps dropped (their pools meet in the spill row), nothing outside the log written"""
    hip = mods
    c = hc.case('solid')
    grid, mat, packs = hc.setup(hip, c)
    lv = hip.HistoryLevels(*hc.LEVELS)
    prm = hip.Params(hc.DT_A, hc.THETA)
    T0 = np.array(c['T0'])
    traj = [T0]
    T = hip.to_device(T0)
    for _ in range(5):
        T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=hc.TINF)
        traj.append(np.asarray(T))
    segs = [(hc.DT_A, 5, None)]
    states, pools, times, t_end = hc.record_trajectory(hip.ThermalHistory, lv, c, traj, clock='run', segments=segs)
    assert all(p['cells'] > 0 for p in pools)
    h = hip.ThermalHistory(grid, lv, capacity=3, T=hip.to_device(T0))
    assert h._log_store.numel() == 4 * 8 + 2 * h.LOG_GUARD
    got = hip.StagedStepper(grid, mat, prm, packs, hc.TINF, history=h).run(hip.to_device(T0), 5)
    assert np.array_equal(np.asarray(got), traj[-1])
    rows = hc.pool_rows(pools)
    assert np.array_equal(_log_rows(h, 3), rows[:3])
    spill = h.d_log.cpu().numpy().reshape(4, 8)[3]
    assert spill[0] == rows[3:, 0].sum() and np.array_equal(spill[1:4], rows[3:, 1:4].min(axis=0)) \
        and np.array_equal(spill[4:7], rows[3:, 4:7].max(axis=0)) and spill[7] == 0
    assert _guards_intact(h)
    mp = h.melt_pool()
    assert mp['dropped'] == 2 and h.slot == 5 and len(mp['cells']) == 3 and np.array_equal(mp['t'], np.array(times[:3]))
    _assert_state(h, states[-1], 'overflow')                      # the fields do not depend on the log
    h.reset(hip.to_device(T0))
    assert h.slot == 0 and h.melt_pool()['dropped'] == 0 and len(h.melt_pool()['cells']) == 0
    empty = np.array([0] + [2 ** 31 - 1] * 3 + [-1] * 3 + [0], dtype=np.int32)
    assert all(np.array_equal(r, empty) for r in h.d_log.cpu().numpy().reshape(4, 8))
    assert _guards_intact(h)


def test_masks_and_births(mods):
    hip = mods
    c = hc.case('holes')
    grid, mat, packs = hc.setup(hip, c)
    mask = np.array(c['mask'])
    lv = hip.HistoryLevels(*hc.LEVELS)
    prm = hip.Params(hc.DT_B, hc.THETA)
    T0 = np.array(c['T0'])
    h = hip.ThermalHistory(grid, lv, capacity=16, T=hip.to_device(T0))
    # markers on every off-mask cell of all three fields: no launch of the recorder writes off the mask
    import torch
    off = torch.from_numpy(~mask).to(h.d_peak.device)
    for f, v in ((h.d_peak, 7.5), (h.d_t_hi, 8.5), (h.d_t_lo, 9.5)):
        f[off] = v
    state = hip.ThermalHistory.seed_reference(hc.empty_state(c['shape']), T0, mask)
    T, t = hip.to_device(T0), 0.0
    for n in range(8):
        Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=hc.TINF, history=h)
        state, _ = hip.ThermalHistory.record_reference(state, np.asarray(T), np.asarray(Tn), mask, t, hc.DT_B, lv)
        t = t + hc.DT_B
        T = Tn
    assert np.isfinite(state[1]).any() and np.isfinite(state[2]).any()
    for got, want, v in zip(_state(h), state, (7.5, 8.5, 9.5)):
        assert (got[~mask] == v).all() and _same(got[mask], want[mask])
    # a birth: cells join the mask at the deposit temperature, others leave it
    born, gone = np.argwhere(~mask)[::5], np.argwhere(mask & np.isfinite(state[1]))[::7]
    m2 = mask.copy()
    m2[tuple(born.T)] = True
    m2[tuple(gone.T)] = False
    assert len(born) and len(gone)
    grid.mask = m2
    with pytest.raises(ValueError, match='sync_mask'):
        h.record(T, hip.to_device(T0), hc.DT_B)
    with pytest.raises(ValueError, match='sync_mask'):
        hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=hc.TINF, history=h)
    with pytest.raises(ValueError, match='sync_mask'):
        hip.StagedStepper(grid, mat, prm, packs, hc.TINF, history=h).run(T, 2)
    T[tuple(born.T)] = 1500.0
    h.sync_mask(T)
    kept = tuple(np.where(mask, s, v) for s, v in zip(state, (7.5, 8.5, 9.5)))    # (what the device holds, markers included)
    want = hip.ThermalHistory.seed_reference(kept, np.asarray(T), m2, m2 & ~mask)
    _assert_state(h, want, 'sync_mask')
    got = _state(h)
    assert (got[0][tuple(born.T)] == 1500.0).all() and np.isnan(got[1][tuple(born.T)]).all()
    assert all(np.isnan(g[tuple(gone.T)]).all() for g in got)
    h.sync_mask(T)                                               # nothing changed: nothing happens
    _assert_state(h, want, 'sync_mask again')
    # what the recorder refuses
    other = hip.Grid3D(*c['shape'], hc.DX, m2)
    with pytest.raises(ValueError, match='another grid'):
        hip.StagedStepper(other, mat, prm, packs, hc.TINF, history=h)
    with pytest.raises(TypeError):
        hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=hc.TINF, history=lv)
    with pytest.raises(ValueError, match="grid's layout"):
        h.record(T0, T, hc.DT_B)
    with pytest.raises(TypeError):
        hip.ThermalHistory(grid, hc.LEVELS)
    with pytest.raises(ValueError, match='capacity'):
        hip.ThermalHistory(grid, lv, capacity=0)


def test_a_brick_whose_peak_is_t_lo_holds_no_crossing(mods):
    """16^3 cells at exactly T_lo cool to 300: the workgroup's vote (some old peak ABOVE T_lo) fails, and the definition agrees;
    one cell a hair above T_lo makes the whole brick look, and that cell alone crosses"""
    hip = mods
    shape = (16, 16, 16)
    mask = np.ones(shape, dtype=bool)
    grid = hip.Grid3D(*shape, 1e-3, mask)
    lv = hip.HistoryLevels(800.0, 500.0, 1400.0)
    for bump in (False, True):
        A, B = np.full(shape, 500.0), np.full(shape, 300.0)
        if bump:
            A[3, 4, 5] = np.nextafter(500.0, 1000.0)
        h = hip.ThermalHistory(grid, lv, capacity=2, T=hip.to_device(A))
        h.record(hip.to_device(A), hip.to_device(B), 0.5)
        state = hip.ThermalHistory.seed_reference(hc.empty_state(shape), A, mask)
        want, _ = hip.ThermalHistory.record_reference(state, A, B, mask, 0.0, 0.5, lv)
        _assert_state(h, want, bump)
        assert int(np.isfinite(want[2]).sum()) == (1 if bump else 0) and h.t == 0.5


# ---- the deposition loops -----------------------------------------------------------------------------------------------
def _assert_result(res, state, pools, times, what):
    for key, want in (('T_peak', state[0]), ('t_hi', state[1]), ('t_lo', state[2]), ('cooling_time', state[2] - state[1])):
        assert _same(res[key], want), (what, key)
    mp = res['melt_pool']
    assert mp['dropped'] == 0 and len(mp['cells']) == len(pools)
    rows = hc.pool_rows(pools)
    assert np.array_equal(mp['cells'], rows[:, 0]) and np.array_equal(mp['lo'], rows[:, 1:4]) and np.array_equal(mp['hi'], rows[:, 4:7])
    assert np.array_equal(mp['t'], np.array(times))


def test_run_single_track_with_history(mods):
    """waam.run_single_track on the small plate of the single-track tests: columns of 20 sub-steps (graph path) and, with a larger
    dt and the latent heat, of 4 (step by step), against the column loop written here with single steps and the definition"""
    hip = mods
    from adi_thermal_fields_amd import waam
    TH = hip.ThermalHistory
    shape, dx = (10, 9, 8), 1e-3
    plate = np.zeros(shape, dtype=bool)
    plate[:, :, :4] = True
    box = (3, 7, 4, 7, 3)
    x0, x1, z0, z1, ncol = box
    Tinf, T_track, theta, t_step, hh = 25.0, 1500.0, 0.5, 0.4, 10.0
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    lv = hip.HistoryLevels(800.0, 500.0, 1400.0)
    robin = {f: hh for f in hc.FACES}
    for dt, with_phase in ((0.02, False), (0.1, True)):
        out = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), hh, Tinf, T_track, theta, dt, t_step,
                                    phase_change=law if with_phase else None, history=lv)
        assert len(out) == (3 if with_phase else 2) and isinstance(out[-1], dict)
        n_sub = max(1, int(math.ceil(t_step / dt)))
        assert (n_sub >= waam.GRAPH_MIN_NSUB) == (dt == 0.02)
        mask = plate.copy()
        grid, mat, prm = hip.Grid3D(*shape, dx, mask.copy()), hip.Material(RHO, CP, K), hip.Params(t_step / n_sub, theta)
        T = hip.to_device(np.full(shape, Tinf))
        ph = hip.PhaseField(grid, mat, law, T=T) if with_phase else None
        state = TH.seed_reference(hc.empty_state(shape), np.asarray(T), mask)
        pools, times, t = [], [], 0.0
        for yi in range(ncol):
            old = mask.copy()
            mask[x0:x1, yi:yi + 1, z0:z1] = True
            grid.mask = mask.copy()
            packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=robin, robin_Tinf=Tinf)
            T[x0:x1, yi:yi + 1, z0:z1] = T_track
            state = TH.seed_reference(state, np.asarray(T), mask, mask & ~old)
            if ph is not None:
                ph.sync_mask(T)
            t0 = t
            for i in range(n_sub):
                Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf, phase=ph)
                t_n = t0 + i * prm.dt if dt == 0.02 else t             # the graph path counts from the run's start
                state, pool = TH.record_reference(state, np.asarray(T), np.asarray(Tn), mask, t_n, prm.dt, lv)
                t = t0 + (i + 1) * prm.dt if dt == 0.02 else t_n + prm.dt
                pools.append(pool)
                times.append(t)
                T = Tn
        assert np.array_equal(out[0], np.asarray(T)), dt
        if with_phase:
            assert np.array_equal(out[1], np.asarray(ph.liquid_fraction))
        assert np.isfinite(state[1]).any() and np.isfinite(state[2]).any() and np.isnan(state[2][mask]).any()
        _assert_result(out[-1], state, pools, times, dt)
    with pytest.raises(ValueError, match='device loop'):
        waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), hh, Tinf, T_track, theta, 0.1, t_step, device_resident=False,
                              history=lv)


def test_run_layer_birth_with_history(mods):
    """waam.run_layer_birth on the 12 x 10 x 14 head of tests/test_phase_gpu.py, born at 1500 degrees, segments shorter and longer
    than GRAPH_MIN_NSUB, against the same event loop written here with single steps and the definition; the levels sit where
    this short run cools through (1450 / 1395; pool: 1440)"""
    hip = mods
    from adi_thermal_fields_amd import waam
    TH = hip.ThermalHistory
    import torch
    shape, dx = (12, 10, 14), 1e-3
    full = waam.synthetic_head_mask(*shape)
    layers = waam.plan_layers(full, 2)
    tb = waam.birth_times(full, layers, dx, bead_width=4e-3, scan_speed=8e-3)
    t_out = [tb[-1] + 6.0 * (tb[-1] - tb[-2])]
    Tinf, Ts, theta, cfl, hh = 25.0, 1500.0, 0.5, 2.0, 40.0
    lv = hip.HistoryLevels(1450.0, 1395.0, 1440.0)
    dt_cap = cfl * dx * dx / KAPPA
    sched = list(waam.layer_birth_schedule(tb, t_out))
    nsubs = [max(1, int(math.ceil(a / dt_cap))) for w, a in sched if w == 'advance']
    assert max(nsubs) >= waam.GRAPH_MIN_NSUB and min(nsubs) < waam.GRAPH_MIN_NSUB, nsubs
    got, nsteps, res = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), hh, Tinf, Ts, theta, cfl, layers, tb, t_out, history=lv)
    # the loop of the driver with its own device calls for births and packs, single steps, and the definition
    mask = np.zeros(shape, dtype=bool)
    grid, mat = hip.Grid3D(*shape, dx, mask), hip.Material(RHO, CP, K)
    T = hip.to_device(np.full(shape, Tinf))
    d_full = grid.layout.to_layout(full, torch.uint8)
    d_act = grid.layout.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    bpacks = hip.BirthPacks(grid, mat, robin_h={f: hh for f in hc.FACES})
    packs = bpacks.packs
    state = TH.seed_reference(hc.empty_state(shape), np.asarray(T), mask)
    pools, times, t, want_steps = [], [], 0.0, 0
    for what, arg in sched:
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = hip.Params(max(arg / nsub, 1e-15), theta)
            run = nsub >= waam.GRAPH_MIN_NSUB
            t0 = t
            for i in range(nsub):
                Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
                t_n = t0 + i * prm.dt if run else t
                state, pool = TH.record_reference(state, np.asarray(T), np.asarray(Tn), mask, t_n, prm.dt, lv)
                t = t0 + (i + 1) * prm.dt if run else t_n + prm.dt
                pools.append(pool)
                times.append(t)
                T = Tn
            want_steps += nsub
        elif what == 'advance':
            t = t + arg                                          # nothing active yet: the global time moves on all the same
        elif what == 'birth':
            ks, ke = layers[arg]
            hip.birth_planes(T, d_act, d_full, grid, ks, ke + 1, Ts)
            grid.set_mask_device(d_act, ks - 1 if ks > 0 else 0, min(shape[2], ke + 2), all_solid=False)
            packs = bpacks.update(ks - 1, ke + 2)
            old = mask.copy()
            mask[:, :, ks:ke + 1] |= full[:, :, ks:ke + 1]
            state = TH.seed_reference(state, np.asarray(T), mask, mask & ~old)
    assert nsteps == want_steps == len(pools)
    assert np.array_equal(got, np.asarray(T))
    assert np.isfinite(state[1]).any() and np.isfinite(state[2]).any() and np.isnan(state[2][mask]).any()
    assert max(p['cells'] for p in pools) > 0 and min(p['cells'] for p in pools) == 0
    _assert_result(res, state, pools, times, 'layer birth')
    assert times[0] > tb[0]                                       # the log's clock is the global time, not the steps' sum
    with pytest.raises(ValueError, match='device loop'):
        waam.run_layer_birth(hip, full, dx, (RHO, CP, K), hh, Tinf, Ts, theta, cfl, layers, tb, t_out, history=lv,
                             device_loop=False)
