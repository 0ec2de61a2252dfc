"""GPU: the solidification recorder on the device -- adi_solid_record / adi_solid_seed through SolidificationRecord, the
`solidification=` argument of adi_step_numba_coeff / StagedStepper and of the waam loops -- against the definition,
SolidificationRecord.record_reference, fed with the fields of the same run without a recorder.

Bars: t_solid, cooling_rate and g2 np.array_equal with NaN in the same places (IEEE subtract / divide / multiply / add in one
fixed order on both sides, contraction off); the T trajectory with the recorder bit-identical to the one without; graph replay
against the same launches issued one by one: bit-identical.  The accessors G = sqrt(g2) and R = cooling_rate / G are formed by
torch on the device: one correctly rounded operation more each, held to 1 and 2 units in the last place of the host's."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import solidification_cases as sc  # noqa: E402
from solidification_cases import CP, K, KAPPA, RHO, T_FREEZE  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


VARIANTS = [('holes', None), ('holes', sc.PADDED['holes']), ('solid', None)]
IDS = ['holes', 'holes_padded', 'solid']


def _pad(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _state(r):
    return np.asarray(r.t_solid), np.asarray(r.cooling_rate), np.asarray(r.g2)


def _assert_state(r, want, what):
    for name, got, w in zip(('t_solid', 'cooling_rate', 'g2'), _state(r), want):
        assert _same(got, w), (what, name, int((~((got == w) | (np.isnan(got) & np.isnan(w)))).sum()))


def _trajectory(hip, c, grid, mat, packs, on_step=None, **kw):
    """the case with single launches, every field downloaded; the source segments in their field form"""
    T = hip.to_device(np.array(c['T0']))
    traj = [np.asarray(T)]
    for dt, n, S in c['segments']:
        prm = hip.Params(dt, sc.THETA)
        d_S = None if S is None else hip.to_device(np.array(S))
        for _ in range(n):
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=sc.TINF, S=d_S, **kw)
            traj.append(np.asarray(T))
            if on_step is not None:
                on_step(len(traj) - 1)
    return traj


_plain = {}


def _plain_run(hip, monkeypatch, name, phys):
    """(case, its trajectory on the device without a recorder, the definition's states over it with single-step clocks, the end
    time): computed once per variant, never modified"""
    _pad(monkeypatch, hip, phys)
    if (name, phys) not in _plain:
        c = sc.case(name)
        grid, mat, packs = sc.setup(hip, c)
        traj = _trajectory(hip, c, grid, mat, packs)
        for a in traj:
            a.setflags(write=False)
        sc.assert_conditions(c, traj)                              # the case reaches what it claims, on the device's own fields
        states, t_end = sc.record_trajectory(hip.SolidificationRecord, c, traj, clock='step')
        _plain[(name, phys)] = (c, traj, states, t_end)
    return _plain[(name, phys)]


def _setup(hip, c, name, phys):
    grid, mat, packs = sc.setup(hip, c)
    if phys is not None:
        assert grid.layout.padded and grid.layout.pd[:3] == phys
    else:
        assert not grid.layout.padded
    if name == 'solid':
        assert grid.all_solid                                      # the flags summary says all-solid: no flags are streamed
    return grid, mat, packs


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_kernel_against_the_definition(mods, monkeypatch, name, phys):
    hip = mods
    c, plain, states, t_end = _plain_run(hip, monkeypatch, name, phys)
    grid, mat, packs = _setup(hip, c, name, phys)
    rec = hip.SolidificationRecord(grid, T_FREEZE, T=hip.to_device(np.array(c['T0'])))
    _assert_state(rec, states[0], 'seed')
    ptrs = rec.graph_key()

    def on_step(n):
        _assert_state(rec, states[n], 'step %d' % n)
    with_rec = _trajectory(hip, c, grid, mat, packs, on_step=on_step, solidification=rec)
    for n, (a, b) in enumerate(zip(plain, with_rec)):
        assert np.array_equal(a, b), n                            # the recorder never touches T
    assert rec.t == t_end and ptrs == rec.graph_key()
    assert int(rec.d_block.cpu()[2].item()) == 1                   # (single records: each sets n = 0 and ticks once)
    # the accessors: sqrt and the quotient, one rounding each on top of the stored numbers
    ts, rate, g2 = states[-1]
    frozen = np.isfinite(g2)
    assert frozen.sum() > 50
    with np.errstate(divide='ignore', invalid='ignore'):
        G_want = np.sqrt(g2)
        R_want = rate / G_want
    G, R = np.asarray(rec.G), np.asarray(rec.R)
    assert np.array_equal(np.isnan(G), ~frozen) and np.array_equal(np.isnan(R), ~frozen)
    ulp = 2.0 ** -52
    assert np.all(np.abs(G[frozen] - G_want[frozen]) <= ulp * G_want[frozen])
    fin = frozen & (G_want > 0.0)
    assert np.all(np.abs(R[fin] - R_want[fin]) <= 2 * ulp * R_want[fin]) and np.isinf(R[frozen & ~fin]).all()


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_no_stray_writes(mods, monkeypatch, name, phys):
    """every word of the three state arrays (plane padding and the cells outside the logical box included) holds a marker of its
    own before a record launch; afterwards every word but those of the freezing cells holds it bit for bit"""
    import torch
    hip = mods
    c, plain, states, _ = _plain_run(hip, monkeypatch, name, phys)
    grid, mat, packs = _setup(hip, c, name, phys)
    n = max(range(1, len(plain)), key=lambda s: sc.freezing(c, plain[s - 1], plain[s]).sum())
    fz = sc.freezing(c, plain[n - 1], plain[n])
    assert n >= 2 and fz.sum() > 10
    rec = hip.SolidificationRecord(grid, T_FREEZE, T=hip.to_device(plain[n - 2]))
    rec.record(hip.to_device(plain[n - 2]), hip.to_device(plain[n - 1]), sc.DT_A)     # (the brick words of step n's input)
    numel = rec._flat[0].numel()
    marks = [torch.arange(numel, dtype=torch.float64, device=rec._flat[0].device) + 1e9 * (f + 1) for f in range(3)]
    for flat, m in zip(rec._flat, marks):
        flat.copy_(m)
    t_n = rec.t
    rec.record(hip.to_device(plain[n - 1]), hip.to_device(plain[n]), sc.DT_B)
    sx, pz = grid.layout.strides[:2]
    idx = np.argwhere(fz)
    at = torch.from_numpy(idx[:, 0] * sx + idx[:, 1] * pz + idx[:, 2]).to(rec._flat[0].device)
    marked = {name_: np.where(fz, np.nan, 0.0) for name_ in ('t_solid', 'cooling_rate', 'g2')}
    want = hip.SolidificationRecord.record_reference(tuple(marked.values()), plain[n - 1], plain[n], c['mask'], t_n, sc.DT_B,
                                                     sc.DX, T_FREEZE)
    for flat, m, got, w in zip(rec._flat, marks, _state(rec), want):
        keep = torch.ones(numel, dtype=torch.bool, device=flat.device)
        keep[at] = False
        assert torch.equal(flat[keep], m[keep])                   # nothing but the freezing cells was written
        assert np.array_equal(got[fz], w[fz]) and np.isfinite(got[fz]).all()


@pytest.mark.parametrize('axis', [0, 2])
def test_births_above_t_freeze_in_cold_bricks(mods, axis):
    """a bar of cells is born at 1500 degrees inside a cold body, across the planes 15 | 16 and 31 | 32 of `axis`: three bricks
    whose words were clear.  sync_mask must set them, or the next step -- which cools the bar's skin through T_freeze -- is
    not looked at"""
    hip = mods
    shape = [8, 8, 8]
    shape[axis] = 36
    shape = tuple(shape)
    bar = [slice(2, 6)] * 3
    bar[axis] = slice(14, 34)
    bar = tuple(bar)
    mask0 = np.ones(shape, dtype=bool)
    mask0[bar] = False
    grid, mat = hip.Grid3D(*shape, sc.DX, mask0.copy()), hip.Material(RHO, CP, K)
    robin = {f: sc.H for f in sc.FACES}
    prm = hip.Params(sc.DT_B, sc.THETA)
    packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=robin)
    SR = hip.SolidificationRecord
    T0 = np.full(shape, sc.TINF)
    rec = SR(grid, T_FREEZE, T=hip.to_device(T0), t=2.0)
    T = hip.adi_step_numba_coeff(hip.to_device(T0), grid, mat, prm, packs, Tinf=sc.TINF, solidification=rec)
    assert not rec.d_hot.cpu().numpy().any() and np.isnan(_state(rec)[0]).all()
    state = SR.seed_reference(sc.empty_state(shape), T0, mask0)
    mask1 = np.ones(shape, dtype=bool)
    grid.mask = mask1.copy()
    packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=robin)
    with pytest.raises(ValueError, match='sync_mask'):
        hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=sc.TINF, solidification=rec)
    with pytest.raises(ValueError, match='sync_mask'):
        hip.StagedStepper(grid, mat, prm, packs, sc.TINF, solidification=rec)
    T[bar] = 1500.0
    rec.sync_mask(T)
    words = rec.d_hot.cpu().numpy().reshape([(n + 15) // 16 for n in grid.layout.pd[:3]])
    assert words.sum() == 3 and words[0, 0, 0] == 1                # the three bricks of the bar, and only they
    A = np.asarray(T)
    state = SR.seed_reference(state, A, mask1, mask1 & ~mask0)
    _assert_state(rec, state, 'sync_mask')
    t_n = rec.t
    Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=sc.TINF, solidification=rec)
    B = np.asarray(Tn)
    fz = mask1 & (A > T_FREEZE) & (B <= T_FREEZE)
    along = np.argwhere(fz)[:, axis]
    assert (along <= 15).any() and ((along >= 16) & (along <= 31)).any() and (along >= 32).any()
    assert t_n == 2.0 + sc.DT_B
    state = SR.record_reference(state, A, B, mask1, t_n, sc.DT_B, sc.DX, T_FREEZE)
    _assert_state(rec, state, 'the step after the birth')
    assert np.array_equal(np.isfinite(_state(rec)[0]), fz)
    rec.sync_mask(Tn)                                             # nothing changed: nothing happens
    _assert_state(rec, state, 'sync_mask again')
    # what the recorder refuses
    other = hip.Grid3D(*shape, sc.DX, mask1)
    with pytest.raises(ValueError, match='another grid'):
        hip.StagedStepper(other, mat, prm, packs, sc.TINF, solidification=rec)
    with pytest.raises(TypeError):
        hip.adi_step_numba_coeff(Tn, grid, mat, prm, packs, Tinf=sc.TINF, solidification=T_FREEZE)
    with pytest.raises(ValueError, match="grid's layout"):
        rec.record(A, Tn, sc.DT_B)
    with pytest.raises(ValueError):
        SR(grid, float('nan'))


def _hist_state(h):
    return (np.asarray(h.T_peak), np.asarray(h.t_hi), np.asarray(h.t_lo), h.d_log.cpu().numpy().copy(), h.t, h.slot)


def test_the_step_is_unchanged_with_phase_history_and_material(mods):
    """the launches of the recorder come last and write none of the step's fields: with a moving source, the surface loss, the
    latent heat and the history (then with the material law and the history; the source goes off after five steps) the T trajectory, the liquid fraction and the
    history's own state are bit-identical with and without `solidification=`, and the record is the definition's"""
    hip = mods
    import matlaw_cases as mc
    shape, dx = (24, 16, 16), 5e-4
    dt, theta, Tinf = 2.0 * dx * dx / KAPPA, 0.5, 25.0
    mask = np.ones(shape, dtype=bool)
    mask[:, :, 12:] = False
    mask[8:20, 6:10, 12:14] = True
    T0 = np.where(mask, 900.0, Tinf)
    src = hip.GoldakSource(power=900.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                           origin=(7 * dx, 8 * dx, 14 * dx), velocity=0.02, travel_axis=0, travel_sign=1, depth_axis=2)
    lv = hip.HistoryLevels(950.0, 920.0, 1450.0)
    T_f = 1100.0                                                  # (between the history's levels and the pool)
    nst, n_on = 16, 5                                             # the source is on for five steps, then the pool freezes
    c = dict(shape=shape, mask=mask, segments=[(dt, nst, None)])
    grid = hip.Grid3D(*shape, dx, mask)
    steel = mc.steel(hip.MaterialLaw)
    for combo in ('phase', 'material'):
        if combo == 'phase':
            mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, theta)
            lp = hip.LossPacks(grid, mat, hip.SurfaceLoss(h=15.0, emissivity=0.8), Tinf)
            ph = hip.PhaseField(grid, mat, hip.PhaseChange(2.7e5, 1400.0, 1450.0), T=hip.to_device(T0))
            packs, kw = lp.packs, dict(surface_loss=lp, phase=ph)
        else:
            nm = hip.NonlinearPacks(grid, RHO, steel, Tinf, loss=hip.SurfaceLoss(h=15.0, emissivity=0.8))
            mat, prm = nm.mat, hip.Params(2.0 * dx * dx * RHO * steel.cp_ref / steel.k_ref, theta)
            ph, packs, kw = None, nm.packs, dict(material=nm)
        runs = {}
        for with_rec in (False, True):
            if ph is not None:
                ph.seed(hip.to_device(T0))
            h = hip.ThermalHistory(grid, lv, capacity=nst, T=hip.to_device(T0))
            rec = hip.SolidificationRecord(grid, T_f, T=hip.to_device(T0)) if with_rec else None
            st = hip.StagedStepper(grid, mat, prm, packs, Tinf, source=src, history=h, solidification=rec, **kw)
            T, traj = hip.to_device(T0), [T0]
            for i in range(nst):
                src.power = 900.0 if i < n_on else 0.0
                T = st.step(T, t=i * prm.dt)
                traj.append(np.asarray(T))
            runs[with_rec] = (traj, _hist_state(h), None if ph is None else np.asarray(ph.liquid_fraction), rec)
        (ta, ha, fa, _), (tb, hb, fb, rec) = runs[False], runs[True]
        for n, (a, b) in enumerate(zip(ta, tb)):
            assert np.array_equal(a, b), (combo, n)
        assert all(_same(a, b) for a, b in zip(ha, hb)), combo
        assert fa is None or np.array_equal(fa, fb)
        c['segments'] = [(prm.dt, nst, None)]
        states, t_end = sc.record_trajectory(hip.SolidificationRecord, c, ta, clock='step', T_freeze=T_f, dx=dx)
        print(combo, 'max T %.0f' % max(a.max() for a in ta), 'frozen cells', int(np.isfinite(states[-1][0]).sum()))
        assert np.isfinite(states[-1][0]).sum() > 0 and max(a.max() for a in ta) > T_f    # a pool that freezes behind the source
        _assert_state(rec, states[-1], combo)
        assert rec.t == t_end
    # solidification=None is the step as it was
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, theta)
    packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h={f: 15.0 for f in sc.FACES})
    assert np.array_equal(np.asarray(hip.adi_step_numba_coeff(hip.to_device(T0), grid, mat, prm, packs, Tinf=Tinf)),
                          np.asarray(hip.adi_step_numba_coeff(hip.to_device(T0), grid, mat, prm, packs, Tinf=Tinf,
                                                              solidification=None)))


def test_graph_replay(mods, monkeypatch):
    """StagedStepper.run through the graph against the same launches one by one, over two consecutive runs with different t0
    (the clock is the recorder's, not t0): fields and clock bit-identical, and both equal to the definition over the stepper's
    own single steps.  From the field just after the pulse: 2 steps of one dt (one replay), then 3 of another (a replay and a
    tail step); cells freeze in both runs.  snapshot / restore round-trips"""
    hip = mods
    c, plain, _, _ = _plain_run(hip, monkeypatch, 'holes', None)
    grid, mat, packs = _setup(hip, c, 'holes', None)
    segs = [(sc.DT_A, 2, None), (sc.DT_B, 3, None)]
    T0 = np.array(plain[1])
    traj = [T0]
    T = hip.to_device(T0)
    for dt, n, _ in segs:
        st = hip.StagedStepper(grid, mat, hip.Params(dt, sc.THETA), packs, sc.TINF)
        for _ in range(n):
            T = st.step(T)
            traj.append(np.asarray(T))
    cc = dict(c, segments=segs)
    states, t_end = sc.record_trajectory(hip.SolidificationRecord, cc, traj, t=1.5, clock='run')
    n_a = int(np.isfinite(states[2][0]).sum())
    assert n_a > 0 and int(np.isfinite(states[5][0]).sum()) > n_a  # cells freeze in both runs
    rec = hip.SolidificationRecord(grid, T_FREEZE, T=hip.to_device(T0), t=1.5)
    sa = hip.StagedStepper(grid, mat, hip.Params(sc.DT_A, sc.THETA), packs, sc.TINF, solidification=rec)
    sb = hip.StagedStepper(grid, mat, hip.Params(sc.DT_B, sc.THETA), packs, sc.TINF, solidification=rec)
    res = {}
    for how in ('graph', 'graph again', 'launches'):
        rec.reset(hip.to_device(T0), t=1.5)
        T = sa.run(hip.to_device(T0), 2, graph=how != 'launches', t0=0.3)
        assert rec.t == 1.5 + 2 * sc.DT_A
        _assert_state(rec, states[2], how)
        snap = rec.snapshot()
        Tb = sb.run(T, 3, graph=how != 'launches', t0=7.0)
        assert rec.t == t_end
        _assert_state(rec, states[5], how)
        assert np.array_equal(np.asarray(Tb), traj[-1])
        res[how] = (np.asarray(Tb),) + _state(rec) + (rec.d_hot.cpu().numpy().copy(), rec.t)
        rec.restore(snap)                                          # back to the end of the first run, brick words and clock too
        assert rec.t == 1.5 + 2 * sc.DT_A
        _assert_state(rec, states[2], how + ', restored')
        sb.run(T, 3, graph=how != 'launches', t0=7.0)
        _assert_state(rec, states[5], how + ', again from the snapshot')
    assert sa.captures == 1 and sb.captures == 1
    for how in ('graph again', 'launches'):
        for a, b in zip(res['graph'], res[how]):
            assert _same(a, b), how
    # another T_freeze: by value in the launch, so another graph, and the new level is the one at work
    rec.T_freeze = 1200.0
    rec.reset(hip.to_device(T0), t=1.5)
    sa.run(hip.to_device(T0), 2)
    assert sa.captures == 2
    want, _ = sc.record_trajectory(hip.SolidificationRecord, dict(c, segments=segs[:1]), traj[:3], t=1.5, clock='run', T_freeze=1200.0)
    _assert_state(rec, want[2], 'another T_freeze')
    assert not _same(want[2][0], states[2][0])


# ---- the deposition loops -----------------------------------------------------------------------------------------------
def _assert_result(res, state, what):
    ts, rate, g2 = state
    with np.errstate(divide='ignore', invalid='ignore'):
        G = np.sqrt(g2)
        R = rate / G
    assert sorted(res) == ['G', 'R', 'cooling_rate', 't_solid']
    for key, want in (('t_solid', ts), ('cooling_rate', rate), ('G', G), ('R', R)):
        assert _same(res[key], want), (what, key)


def test_run_single_track_with_solidification(mods):
    """waam.run_single_track on the small plate of the single-track tests: columns of 20 sub-steps (graph path) and, with a larger
    dt, the latent heat and the history, of 4 (step by step), against the column loop written here with single steps and the
    definition; the usual return values are those of the run without a recorder"""
    hip = mods
    from adi_thermal_fields_amd import waam
    SR = hip.SolidificationRecord
    shape, dx = (10, 9, 8), 1e-3
    plate = np.zeros(shape, dtype=bool)
    plate[:, :, :4] = True
    box = (3, 7, 4, 7, 3)
    x0, x1, z0, z1, ncol = box
    Tinf, T_track, theta, t_step, hh, T_f = 25.0, 1500.0, 0.5, 0.4, 10.0, 1400.0
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    lv = hip.HistoryLevels(800.0, 500.0, 1400.0)
    robin = {f: hh for f in sc.FACES}
    for dt, extras in ((0.02, False), (0.1, True)):
        kw = dict(phase_change=law, history=lv) if extras else {}
        usual = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), hh, Tinf, T_track, theta, dt, t_step, **kw)
        out = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), hh, Tinf, T_track, theta, dt, t_step, solidification=T_f,
                                    **kw)
        if extras:
            assert len(out) == 4 and isinstance(out[2], dict) and 'T_peak' in out[2]      # after history's dict
            assert np.array_equal(out[0], usual[0]) and np.array_equal(out[1], usual[1])
            assert all(_same(out[2][k], usual[2][k]) for k in ('T_peak', 't_hi', 't_lo', 'cooling_time'))
        else:
            assert len(out) == 2 and np.array_equal(out[0], usual)
        n_sub = max(1, int(math.ceil(t_step / dt)))
        assert (n_sub >= waam.GRAPH_MIN_NSUB) == (dt == 0.02)
        mask = plate.copy()
        grid, mat, prm = hip.Grid3D(*shape, dx, mask.copy()), hip.Material(RHO, CP, K), hip.Params(t_step / n_sub, theta)
        T = hip.to_device(np.full(shape, Tinf))
        ph = hip.PhaseField(grid, mat, law, T=T) if extras else None
        state = SR.seed_reference(sc.empty_state(shape), np.asarray(T), mask)
        t = 0.0
        for yi in range(ncol):
            old = mask.copy()
            mask[x0:x1, yi:yi + 1, z0:z1] = True
            grid.mask = mask.copy()
            packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=robin, robin_Tinf=Tinf)
            T[x0:x1, yi:yi + 1, z0:z1] = T_track
            state = SR.seed_reference(state, np.asarray(T), mask, mask & ~old)
            if ph is not None:
                ph.sync_mask(T)
            t0 = t
            for i in range(n_sub):
                Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf, phase=ph)
                t_n = t0 + i * prm.dt if dt == 0.02 else t             # the graph path counts from the run's start
                state = SR.record_reference(state, np.asarray(T), np.asarray(Tn), mask, t_n, prm.dt, dx, T_f)
                t = t0 + (i + 1) * prm.dt if dt == 0.02 else t_n + prm.dt
                T = Tn
        assert np.array_equal(out[0], np.asarray(T)), dt
        assert np.isfinite(state[0]).sum() > 0 and np.isnan(state[0][mask]).any()
        _assert_result(out[-1], state, dt)
    with pytest.raises(ValueError, match='device loop'):
        waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), hh, Tinf, T_track, theta, 0.1, t_step, device_resident=False,
                              solidification=T_f)


def test_run_layer_birth_with_solidification(mods):
    """waam.run_layer_birth on the 12 x 10 x 14 head of tests/test_phase_gpu.py, born at 1500 degrees, segments shorter and longer
    than GRAPH_MIN_NSUB, against the same event loop written here with single steps and the definition"""
    hip = mods
    from adi_thermal_fields_amd import waam
    SR = hip.SolidificationRecord
    import torch
    shape, dx = (12, 10, 14), 1e-3
    full = waam.synthetic_head_mask(*shape)
    layers = waam.plan_layers(full, 2)
    tb = waam.birth_times(full, layers, dx, bead_width=4e-3, scan_speed=8e-3)
    t_out = [tb[-1] + 6.0 * (tb[-1] - tb[-2])]
    Tinf, Ts, theta, cfl, hh, T_f = 25.0, 1500.0, 0.5, 2.0, 40.0, 1420.0
    dt_cap = cfl * dx * dx / KAPPA
    sched = list(waam.layer_birth_schedule(tb, t_out))
    nsubs = [max(1, int(math.ceil(a / dt_cap))) for w, a in sched if w == 'advance']
    assert max(nsubs) >= waam.GRAPH_MIN_NSUB and min(nsubs) < waam.GRAPH_MIN_NSUB, nsubs
    usual = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), hh, Tinf, Ts, theta, cfl, layers, tb, t_out)
    got, nsteps, res = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), hh, Tinf, Ts, theta, cfl, layers, tb, t_out,
                                            solidification=T_f)
    assert len(usual) == 2 and np.array_equal(usual[0], got) and usual[1] == nsteps
    # the loop of the driver with its own device calls for births and packs, single steps, and the definition
    mask = np.zeros(shape, dtype=bool)
    grid, mat = hip.Grid3D(*shape, dx, mask), hip.Material(RHO, CP, K)
    T = hip.to_device(np.full(shape, Tinf))
    d_full = grid.layout.to_layout(full, torch.uint8)
    d_act = grid.layout.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    bpacks = hip.BirthPacks(grid, mat, robin_h={f: hh for f in sc.FACES})
    packs = bpacks.packs
    state = SR.seed_reference(sc.empty_state(shape), np.asarray(T), mask)
    t, want_steps, first = 0.0, 0, None
    for what, arg in sched:
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = hip.Params(max(arg / nsub, 1e-15), theta)
            run = nsub >= waam.GRAPH_MIN_NSUB
            t0 = t
            first = t0 if first is None else first
            for i in range(nsub):
                Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
                t_n = t0 + i * prm.dt if run else t
                state = SR.record_reference(state, np.asarray(T), np.asarray(Tn), mask, t_n, prm.dt, dx, T_f)
                t = t0 + (i + 1) * prm.dt if run else t_n + prm.dt
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
            state = SR.seed_reference(state, np.asarray(T), mask, mask & ~old)
    assert nsteps == want_steps
    assert np.array_equal(got, np.asarray(T))
    assert np.isfinite(state[0]).sum() > 50
    assert np.nanmin(state[0]) > first >= tb[0]                   # the clock is the global time, not the steps' sum
    _assert_result(res, state, 'layer birth')
    with pytest.raises(ValueError, match='device loop'):
        waam.run_layer_birth(hip, full, dx, (RHO, CP, K), hh, Tinf, Ts, theta, cfl, layers, tb, t_out, solidification=T_f,
                             device_loop=False)
