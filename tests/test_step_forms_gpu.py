"""GPU: the four forms of the Cartesian step -- adi_step_numba_coeff with a GoldakSource and with a source field, StagedStepper.step,
StagedStepper.run with plain launches and through the graph -- with surface loss, latent heat, the thermal history and a source
all on, each against the step's launch order SPELLED OUT HERE from the leaf launchers:
    lp.update(T); explicit stage + sweep 0 (one fused launch, or two); src.set_block + the source's correction of sweep 0's
    output; sweep 1; sweep 2; ph.apply(out); h.record(T, out, dt)
and for the field form  lp.update(T); explicit stage with S = src.sample(grid, t + dt/2); sweeps 0, 1, 2; ph.apply; h.record.

Bars: every comparison is np.array_equal (NaN in the same places for the history fields): T after every step, the liquid
fraction, T_peak / t_hi / t_lo, the log rows, the recorder's slot, and its clock and log times against the definition keeping the
clock the way the form does (run: t0 + n*dt; single steps: repeated t + dt).

Shapes: the inputs of tests/history_cases.py (holes mask, hot blob, Robin on every face) at the smallest boxes that take both
branches of the sequence: (20, 18, 35) fused through the GENERAL kernel, odd nz; (64, 16, 32) fused through the tiled FAST kernel,
also with StagedStepper(fused=False); (72, 12, 20), physical box pinned to the logical one, where the fused kernel is not
available (nx >= 64, nz % 16 != 0)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import history_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu

NST, DT = 4, hc.DT_A
CONFIGS = [('general', (20, 18, 35), None), ('fast', (64, 16, 32), None), ('fast_two_launches', (64, 16, 32), False),
           ('no_fused_kernel', (72, 12, 20), None)]


@pytest.fixture(scope='module')
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


def _inputs(shape):
    """the 'holes' case of history_cases on a box of `shape`: (mask, T0, blob)"""
    if shape == hc.SHAPES['holes']:
        c = hc.case('holes')
        return np.array(c['mask']), np.array(c['T0']), c['blob']
    rng = np.random.default_rng(11)
    blob = hc._blob(shape)
    mask = rng.random(shape) > 0.07
    mask[blob] = True
    T0 = np.full(shape, hc.TINF)
    T0[blob] = 1900.0
    for p in [(2, 2, 3), (3, shape[1] - 3, shape[2] - 4), (shape[0] - 3, 3, shape[2] - 6)]:
        mask[p] = True
        T0[p] = 1000.0
    return mask, np.where(mask, T0, hc.TINF), blob


class Rig:
    """grid, packs and the four extras of one shape"""

    def __init__(self, hip, shape):
        self.hip = hip
        self.mask, self.T0, blob = _inputs(shape)
        self.grid = hip.Grid3D(*shape, hc.DX, self.mask.copy())
        self.mat, self.prm = hip.Material(hc.RHO, hc.CP, hc.K), hip.Params(DT, hc.THETA)
        self.lp = hip.LossPacks(self.grid, self.mat, hip.SurfaceLoss(h=hc.H, emissivity=0.8), hc.TINF)
        self.packs = self.lp.packs
        self.law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)            # the blob (1900) cools through the interval
        self.ph = hip.PhaseField(self.grid, self.mat, self.law, T=hip.to_device(self.T0))
        self.lv = hip.HistoryLevels(*hc.LEVELS)
        self.h = hip.ThermalHistory(self.grid, self.lv, capacity=NST + 2, T=hip.to_device(self.T0))
        ctr = [0.5 * (s.start + s.stop) * hc.DX for s in blob]       # inside the blob, travelling along axis 0
        self.src = hip.GoldakSource(power=900.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                                    origin=(ctr[0] - 2 * hc.DX, ctr[1], ctr[2]), velocity=0.02, travel_axis=0, travel_sign=1,
                                    depth_axis=2)
        self.extras = dict(surface_loss=self.lp, phase=self.ph, history=self.h)

    def fresh(self):
        """before every compared run: f and the history as at the start"""
        self.ph.seed(self.hip.to_device(self.T0))
        self.h.reset(self.hip.to_device(self.T0))

    def state(self):
        h = self.h
        return dict(f=np.asarray(self.ph.liquid_fraction), peak=np.asarray(h.T_peak), t_hi=np.asarray(h.t_hi),
                    t_lo=np.asarray(h.t_lo), rows=h.d_log.cpu().numpy().reshape(h.capacity + 1, 8)[:NST].copy(), slot=h.slot)

    def field_at(self, i):
        return self.src.sample(self.grid, i * DT + 0.5 * DT)


def _spelled_out(r, fused, field):
    """NST steps from the leaf launchers, in the order the module's docstring states -> ([T0, T1, ...], state at the end, the
    recorder's clock and log times as single recorded steps keep them)"""
    hip, g, mat, prm, packs = r.hip, r.grid, r.mat, r.prm, r.packs
    r.fresh()
    T = hip.to_device(r.T0).t
    R, U, V = g.layout.empty(), g.layout.empty(), g.layout.empty()
    traj = [r.T0]
    for i in range(NST):
        out = g.layout.empty()
        r.lp.update(T, hc.TINF)
        if field:
            hip._explicit_src_into(T, hip.to_device(r.field_at(i)).t, R, g, mat, prm)
            hip._sweep_into(0, R, U, g, mat, prm, packs[0], hc.TINF)
        else:
            if fused:
                hip._explicit_sweep0_into(T, U, g, mat, prm, packs[0], hc.TINF)
            else:
                R = hip.adi_explicit_rhs(T, g, mat, prm)
                hip._sweep_into(0, R, U, g, mat, prm, packs[0], hc.TINF)
            r.src.set_block(hip._source_block(g), i * DT, DT)
            hip._source_lines0_into(U, g, mat, prm, packs[0], r.src, g)
        hip._sweep_into(1, U, V, g, mat, prm, packs[1], hc.TINF)
        hip._sweep_into(2, V, out, g, mat, prm, packs[2], hc.TINF)
        r.ph.apply(out, packs[2].d_dir_mask if packs[2].has_dir else None)
        r.h.record(T, out, DT)
        T = out
        traj.append(np.asarray(hip.DeviceField(T)))
    return traj, r.state(), r.h.t, r.h.melt_pool()['t']


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check(r, what, got_T, want, clock):
    """T, f, the history fields, the log rows and the slot against the spelled-out sequence; the history fields, the clock and
    the log times against the definition that keeps the clock like the form"""
    traj, state, defs = want
    assert np.array_equal(np.asarray(got_T), traj[-1]), what
    got = r.state()
    for k in ('f', 'peak', 't_hi', 't_lo', 'rows'):
        assert _same(got[k], state[k]), (what, k)
    assert got['slot'] == NST, what
    states, times, t_end = defs[clock]
    for k, w in zip(('peak', 't_hi', 't_lo'), states[-1]):
        assert _same(got[k], w), (what, k, 'definition')
    assert r.h.t == t_end and np.array_equal(r.h.melt_pool()['t'], np.array(times)), what


def _definition(r, traj):
    c = dict(shape=r.grid.shape, mask=r.mask, segments=[(DT, NST, None)])
    out = {}
    for clock in ('step', 'run'):
        states, pools, times, t_end = hc.record_trajectory(r.hip.ThermalHistory, r.lv, c, traj, clock=clock)
        out[clock] = (states, times, t_end)
    return out, pools


@pytest.mark.parametrize('name,shape,fused', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_form_is_the_spelled_out_sequence(hip, monkeypatch, name, shape, fused):
    if name == 'no_fused_kernel':
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx, ny, nz))
    r = Rig(hip, shape)
    g, mat, prm, packs, src = r.grid, r.mat, r.prm, r.packs, r.src
    assert not g.layout.padded
    assert hip.fused_supported(g) == (name != 'no_fused_kernel')
    use_fused = hip.fused_supported(g) if fused is None else fused
    traj, state, t_step, times_step = _spelled_out(r, use_fused, field=False)
    defs, pools = _definition(r, traj)
    # the run is not vacuous, and the spelled-out recorder is the definition's with the clock of single steps
    assert (state['f'] > 0.0).any() and np.isfinite(state['t_hi']).any() and max(p['cells'] for p in pools) > 0
    assert ((state['f'] > 0.0) & (state['f'] < 1.0)).any()
    assert np.array_equal(state['rows'], hc.pool_rows(pools))
    assert t_step == defs['step'][2] and np.array_equal(times_step, np.array(defs['step'][1]))
    want = (traj, state, defs)

    st = hip.StagedStepper(g, mat, prm, packs, hc.TINF, fused=fused, source=src, **r.extras)
    assert st.fused == use_fused
    r.fresh()
    T = hip.to_device(r.T0)
    for i in range(NST):
        T = st.step(T, t=i * DT)
        assert np.array_equal(np.asarray(T), traj[i + 1]), i
    _check(r, 'StagedStepper.step', T, want, 'step')
    for graph in (False, True):
        r.fresh()
        T = st.run(hip.to_device(r.T0), NST, graph=graph, t0=0.0)
        _check(r, 'StagedStepper.run graph=%s' % graph, T, want, 'run')
    assert st.captures == 1
    if fused is not None:
        return                                   # adi_step_numba_coeff takes the fused kernel wherever there is one

    for kind in ('field', 'numpy'):
        r.fresh()
        T = hip.to_device(r.T0) if kind == 'field' else r.T0.copy()
        for i in range(NST):
            before = np.array(T)
            Tn = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=hc.TINF, S=src, t=i * DT, **r.extras)
            assert isinstance(Tn, hip.DeviceField if kind == 'field' else np.ndarray) and Tn is not T
            assert np.array_equal(np.asarray(T), before)                      # the input is left as it was
            assert np.array_equal(np.asarray(Tn), traj[i + 1]), (kind, i)
            T = Tn
        _check(r, 'adi_step_numba_coeff ' + kind, T, want, 'step')

    # the field form: its own spelled-out sequence
    traj_f, state_f, t_f, times_f = _spelled_out(r, False, field=True)
    defs_f, pools_f = _definition(r, traj_f)
    assert (state_f['f'] > 0.0).any() and np.isfinite(state_f['t_hi']).any() and max(p['cells'] for p in pools_f) > 0
    assert t_f == defs_f['step'][2] and np.array_equal(times_f, np.array(defs_f['step'][1]))
    for kind in ('field', 'numpy'):
        r.fresh()
        T = hip.to_device(r.T0) if kind == 'field' else r.T0.copy()
        for i in range(NST):
            S = hip.to_device(r.field_at(i)) if kind == 'field' else r.field_at(i)
            before = np.array(T)
            Tn = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=hc.TINF, S=S, **r.extras)
            assert isinstance(Tn, hip.DeviceField if kind == 'field' else np.ndarray) and Tn is not T
            assert np.array_equal(np.asarray(T), before)
            assert np.array_equal(np.asarray(Tn), traj_f[i + 1]), (kind, i)
            T = Tn
        _check(r, 'adi_step_numba_coeff, source field, ' + kind, T, (traj_f, state_f, defs_f), 'step')


def test_a_foreign_phase_field_is_refused_before_anything_is_launched(hip):
    """adi_step_numba_coeff with the PhaseField of another grid: ValueError, and neither the recorder (fields, log, slot, clock),
    the PhaseField nor the LossPacks' coefficients (which the step's first launch would rewrite) have moved"""
    r = Rig(hip, hc.SHAPES['holes'])
    other = hip.Grid3D(*r.grid.shape, hc.DX, r.mask.copy())
    ph2 = hip.PhaseField(other, r.mat, r.law, T=hip.to_device(r.T0))
    r.lp.update(hip.to_device(np.full(r.grid.shape, hc.TINF)), hc.TINF)      # coefficients of a cold field: T0 would change them
    r.h.reset(hip.to_device(r.T0), t=0.75)
    coeff = [p.d_coeff.clone() for p in r.packs]
    f2, words2 = ph2.snapshot()
    before, log, t = r.state(), r.h._log_store.clone(), r.h.t
    for S in (None, r.src, hip.to_device(r.field_at(0))):
        with pytest.raises(ValueError, match='another grid'):
            hip.adi_step_numba_coeff(hip.to_device(r.T0), r.grid, r.mat, r.prm, r.packs, Tinf=hc.TINF, S=S, surface_loss=r.lp,
                                     phase=ph2, history=r.h)
    after = r.state()
    assert all(_same(before[k], after[k]) for k in before) and after['slot'] == 0
    assert r.h.t == t == 0.75 and bool((r.h._log_store == log).all()) and len(r.h.melt_pool()['t']) == 0
    assert bool((ph2._flat == f2).all()) and bool((ph2.summary == words2).all())
    assert all(bool((p.d_coeff == c).all()) for p, c in zip(r.packs, coeff))
    # ... and the coefficients would have moved: the same call with the grid's own PhaseField rewrites them
    hip.adi_step_numba_coeff(hip.to_device(r.T0), r.grid, r.mat, r.prm, r.packs, Tinf=hc.TINF, surface_loss=r.lp, phase=r.ph,
                             history=r.h)
    assert any(not bool((p.d_coeff == c).all()) for p, c in zip(r.packs, coeff)) and r.h.slot == 1
