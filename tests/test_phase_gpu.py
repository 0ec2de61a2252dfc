"""GPU: latent heat on the device -- adi_phase_apply / adi_phase_seed through PhaseField, the `phase=` argument of
adi_step_numba_coeff / StagedStepper and `phase_change=` of the waam loops -- against the golden vectors of the reference
(tests/golden/make_golden_phase.py) and, where the reference has no vectors, against the corrected loop over the pinned C oracle
that tests/test_phase_cpu.py holds to those vectors.

Bars: the correction on a stored T*: np.array_equal (IEEE multiply / add / divide in one fixed order on both sides, contraction
off); whole sequences T <= 1e-10 relative L-inf, the project's bar, and |f - f_golden| <= 1e-10 max|T| / (Tl - Ts), the same bar
pushed through f = (T - Ts)/dT; graph replay against the same launches issued one by one: bit-identical.  After every step the
phase summary is read back: an entry is 0 exactly when every f of its brick is 0 in memory."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import phase_cases as pc  # noqa: E402
from phase_cases import CP, K, KAPPA, RHO, rel_linf  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


# every golden case on the box the library picks for it, and the cases with partial bricks once more on a padded physical box
# whose rows are whole 16-byte pieces (the 16-byte loads, cells of the box outside the logical grid)
VARIANTS = [('holes', None), ('holes', (12, 8, 16)), ('two_bricks', None), ('two_bricks', (24, 20, 36)), ('refreeze', None)]
IDS = ['holes', 'holes_padded', 'two_bricks', 'two_bricks_padded', 'refreeze']


def _pad(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _setup(hip, c):
    grid = hip.Grid3D(*c['mask'].shape, float(c['dx']), np.array(c['mask']))
    mat = hip.Material(float(c['rho']), float(c['cp']), float(c['k']))
    dm, dv = pc.dir_of(c)
    packs = hip.precompute_coeff_packs_unified(grid, mat, dir_mask=dm, dir_value=dv, robin_h=pc.robin_of(c))
    return grid, mat, packs, dm


def _f_phys(ph):
    """f over the whole physical box, as it is in memory"""
    import torch
    px, py, pz, sx = ph.grid.layout.pd
    return torch.as_strided(ph.f, (px, py, pz), (sx, pz, 1)).cpu().numpy()


def _assert_summary(ph, what):
    """entry == 0 <=> every f of the brick is 0 in memory"""
    f = _f_phys(ph)
    nb = [(n + 15) // 16 for n in f.shape]
    got = ph.summary.cpu().numpy().reshape(nb)
    want = np.zeros(nb, dtype=bool)
    for bi in range(nb[0]):
        for bj in range(nb[1]):
            for bk in range(nb[2]):
                want[bi, bj, bk] = (f[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16, 16 * bk:16 * bk + 16] != 0.0).any()
    assert np.array_equal(got != 0, want), (what, got.ravel().tolist(), want.ravel().tolist())
    return want


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_apply_on_the_stored_fields_is_bit_identical(mods, monkeypatch, name, phys):
    hip, _ = mods
    _pad(monkeypatch, hip, phys)
    c = pc.load(name)
    grid, mat, packs, dm = _setup(hip, c)
    if phys is not None:
        assert grid.layout.padded and grid.layout.pd[:3] == phys
    mask = c['mask']
    law = pc.law_of(c, hip.PhaseChange)
    ph = hip.PhaseField(grid, mat, law, T=hip.to_device(np.array(c['T0'])), dir_mask=dm)
    assert np.array_equal(np.asarray(ph.liquid_fraction), c['f0'])        # the seed: f_eq(T0) on the mask, Dirichlet cells too
    _assert_summary(ph, 'seed')
    ptrs = (ph.f.data_ptr(), ph.summary.data_ptr())
    planted = 0
    for n in range(1, int(c['nsteps']) + 1):
        f_in = np.array(c['f%d' % (n - 1)])
        ph.set_liquid_fraction(f_in)
        bricks = _assert_summary(ph, 'load %d' % n)
        # a marker in the f of an off-mask cell whose brick holds liquid (so that the summary stays true to the memory)
        off = [p for p in np.argwhere(~mask) if bricks[p[0] // 16, p[1] // 16, p[2] // 16]]
        if off:
            i, j, k = (int(v) for v in off[len(off) // 2])
            ph.f[i, j, k] = 7.5
            f_in[i, j, k] = 7.5
            planted += 1
        Tstar = c['Tstar%d' % n]
        T = hip.to_device(np.array(Tstar))
        ph.apply(T)
        gT, gf = np.asarray(T), np.asarray(ph.liquid_fraction)
        want_f = np.where(mask, c['f%d' % n], f_in)
        assert np.array_equal(gT, c['T%d' % n]), (n, int((gT != c['T%d' % n]).sum()), rel_linf(gT, c['T%d' % n]))
        assert np.array_equal(gf, want_f), (n, int((gf != want_f).sum()), float(np.abs(gf - want_f).max()))
        keep = ~mask if dm is None else (~mask | dm)
        rest = mask & (((f_in == 0) & (Tstar <= float(c['T_solidus']))) | ((f_in == 1) & (Tstar >= float(c['T_liquidus']))))
        for sel in (keep, rest):
            assert np.array_equal(gT[sel], Tstar[sel]) and np.array_equal(gf[sel], f_in[sel])
        _assert_summary(ph, 'apply %d' % n)
    assert planted > 0 or name == 'refreeze'                              # (refreeze has no off-mask cell)
    assert ptrs == (ph.f.data_ptr(), ph.summary.data_ptr())


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_sequence_through_the_step(mods, monkeypatch, name, phys):
    """the whole golden sequence through adi_step_numba_coeff(phase=), the source segments in its field form"""
    hip, _ = mods
    _pad(monkeypatch, hip, phys)
    c = pc.load(name)
    grid, mat, packs, dm = _setup(hip, c)
    law = pc.law_of(c, hip.PhaseChange)
    T0 = hip.to_device(np.array(c['T0']))
    T = T0
    ph = hip.PhaseField(grid, mat, law, T=T)
    n = 0
    states = []
    for dt, nsteps, S in pc.segments(c):
        prm = hip.Params(dt, float(c['theta']))
        d_S = None if S is None else hip.to_device(S)
        for _ in range(nsteps):
            prev = T
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=float(c['Tinf']), S=d_S, phase=ph)
            n += 1
            assert T.t.data_ptr() != prev.t.data_ptr()
            eT, ef = rel_linf(np.asarray(T), c['T%d' % n]), float(np.abs(np.asarray(ph.liquid_fraction) - c['f%d' % n]).max())
            print(name, 'step', n, 'T rel L-inf %.3e  |df| %.3e' % (eT, ef))
            assert eT <= 1e-10 and ef <= pc.f_bar(c), (name, n, eT, ef)
            states.append(bool(_assert_summary(ph, 'step %d' % n).any()))
    assert np.array_equal(np.asarray(T0), c['T0'])                         # the input of a step is never modified
    if name == 'refreeze':                                                 # not loaded -> set -> cleared -> set again
        assert states[1] and not states[5] and states[7], states
    if name.startswith('two_bricks'):
        s = ph.summary.cpu().numpy()
        assert (s == 0).any() and (s != 0).any()
    # the NumPy form of the call: host arrays in and out, the same numbers
    ph.seed(T0)
    dt, _, S = pc.segments(c)[0]
    got = hip.adi_step_numba_coeff(np.array(c['T0']), grid, mat, hip.Params(dt, float(c['theta'])), packs, Tinf=float(c['Tinf']),
                                   S=S, phase=ph)
    assert isinstance(got, np.ndarray) and rel_linf(got, c['T1']) <= 1e-10


@pytest.mark.parametrize('name,phys', VARIANTS, ids=IDS)
def test_sequence_through_the_stepper_graph_and_single_launches(mods, monkeypatch, name, phys):
    """StagedStepper.run (graph replay) for the segments without a source field, against the golden vectors; against run() with
    plain launches, against n step() calls and against the stepper without phase= followed by PhaseField.apply, all bit for bit
    in T and f -- the warm-up steps of the capture must not leak into f"""
    hip, _ = mods
    _pad(monkeypatch, hip, phys)
    c = pc.load(name)
    grid, mat, packs, dm = _setup(hip, c)
    law = pc.law_of(c, hip.PhaseChange)
    ph = hip.PhaseField(grid, mat, law)
    first = 0
    for s, (dt, nsteps, S) in enumerate(pc.segments(c)):
        last = first + nsteps
        if S is None:
            prm = hip.Params(dt, float(c['theta']))
            st = hip.StagedStepper(grid, mat, prm, packs, float(c['Tinf']), phase=ph)
            plain = hip.StagedStepper(grid, mat, prm, packs, float(c['Tinf']))
            T_in, f_in = np.array(c['T%d' % first]), np.array(c['f%d' % first])
            res = {}
            for how in ('graph', 'graph again', 'launches', 'steps', 'apply'):
                ph.set_liquid_fraction(f_in)
                T = hip.to_device(T_in)
                if how.startswith('graph'):
                    T = st.run(T, nsteps)
                elif how == 'launches':
                    T = st.run(T, nsteps, graph=False)
                else:
                    for _ in range(nsteps):
                        if how == 'steps':
                            T = st.step(T)
                        else:
                            T = plain.step(T)
                            ph.apply(T, packs[2].d_dir_mask if packs[2].has_dir else None)
                res[how] = (np.asarray(T), np.asarray(ph.liquid_fraction))
                _assert_summary(ph, how)
            assert st.captures == 1
            eT, ef = rel_linf(res['graph'][0], c['T%d' % last]), float(np.abs(res['graph'][1] - c['f%d' % last]).max())
            print(name, 'segment', s, 'T rel L-inf %.3e  |df| %.3e' % (eT, ef))
            assert eT <= 1e-10 and ef <= pc.f_bar(c), (name, s, eT, ef)
            for how in ('graph again', 'launches', 'steps', 'apply'):
                assert np.array_equal(res['graph'][0], res[how][0]) and np.array_equal(res['graph'][1], res[how][1]), how
        first = last


def test_cold_field_is_the_step_without_phase(mods):
    """holes_mixed of the project's golden cases stays below 1000 degrees: with a law that melts at 1400 the result is the step's
    own, bit for bit, f stays 0 and no entry of the summary is set"""
    hip, _ = mods
    import cases
    c = cases.cart_case('holes_mixed')
    assert c['T0'].max() < 1400.0
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    mat, prm = hip.Material(**c['mat']), hip.Params(c['dt'], c['theta'])
    packs = hip.precompute_coeff_packs_unified(grid, mat, dir_mask=c['dir_mask'], dir_value=c['dir_value'], neumann=c['neumann'],
                                               robin_h=c['robin_h'])
    ph = hip.PhaseField(grid, mat, hip.PhaseChange(2.7e5, 1400.0, 1450.0), T=hip.to_device(c['T0']))
    a = b = hip.to_device(c['T0'])
    for _ in range(c['nsteps']):
        a = hip.adi_step_numba_coeff(a, grid, mat, prm, packs, Tinf=c['Tinf'])
        b = hip.adi_step_numba_coeff(b, grid, mat, prm, packs, Tinf=c['Tinf'], phase=ph)
        assert np.array_equal(np.asarray(a), np.asarray(b))
        assert not _f_phys(ph).any() and not ph.summary.cpu().numpy().any()
    st = hip.StagedStepper(grid, mat, prm, packs, c['Tinf'], phase=ph)
    assert np.array_equal(np.asarray(st.run(hip.to_device(c['T0']), c['nsteps'])), np.asarray(a))
    assert not _f_phys(ph).any() and not ph.summary.cpu().numpy().any()


def test_phase_field_refuses_what_it_cannot_correct(mods):
    hip, _ = mods
    c = pc.load('holes')
    grid, mat, packs, dm = _setup(hip, c)
    law = pc.law_of(c, hip.PhaseChange)
    ph = hip.PhaseField(grid, mat, law)
    other = hip.Grid3D(*c['mask'].shape, float(c['dx']), np.array(c['mask']))
    prm = hip.Params(float(c['seg0_dt']), 0.5)
    with pytest.raises(ValueError, match='another grid'):
        hip.StagedStepper(other, mat, prm, packs, 25.0, phase=ph)
    with pytest.raises(ValueError, match='cp'):
        hip.adi_step_numba_coeff(np.array(c['T0']), grid, hip.Material(RHO, 500.0, K), prm, packs, Tinf=25.0, phase=ph)
    with pytest.raises(TypeError):
        hip.adi_step_numba_coeff(np.array(c['T0']), grid, mat, prm, packs, Tinf=25.0, phase=law)
    with pytest.raises(ValueError, match="grid's layout"):
        ph.apply(np.array(c['T0']))
    m2 = np.array(c['mask'])
    m2[4, 3, 5] = not m2[4, 3, 5]
    grid.mask = m2
    with pytest.raises(ValueError, match='sync_mask'):
        ph.apply(hip.to_device(np.array(c['T0'])))
    # copies of the state
    ph2 = hip.PhaseField(grid, mat, law, T=hip.to_device(np.array(c['T0'])))
    snap = ph2.snapshot()
    ph.copy_state_from(ph2)
    assert np.array_equal(_f_phys(ph), _f_phys(ph2)) and np.array_equal(ph.summary.cpu().numpy(), ph2.summary.cpu().numpy())
    ph2.seed(hip.to_device(np.full(c['mask'].shape, 20.0)))
    assert not _f_phys(ph2).any() and not ph2.summary.cpu().numpy().any()
    ph2.restore(snap)
    assert np.array_equal(_f_phys(ph), _f_phys(ph2)) and ph2.summary.cpu().numpy().any()


def test_sync_mask_seeds_the_newborn_cells_only(mods):
    hip, _ = mods
    c = pc.load('holes')
    grid, mat, packs, dm = _setup(hip, c)
    law = pc.law_of(c, hip.PhaseChange)
    mask = np.array(c['mask'])
    T = np.array(c['T0'])
    ph = hip.PhaseField(grid, mat, law, T=hip.to_device(T))
    f_old = np.array(c['f3'])
    ph.set_liquid_fraction(f_old)
    m2 = mask.copy()
    born = np.argwhere(~mask)[::7]
    gone = np.argwhere(mask & (f_old > 0))[::9]
    m2[tuple(born.T)] = True
    m2[tuple(gone.T)] = False
    grid.mask = m2
    ph.sync_mask(hip.to_device(T))
    want = np.where(m2, f_old, 0.0)
    want[tuple(born.T)] = law.f_eq(T)[tuple(born.T)]
    assert len(born) and len(gone) and want[tuple(born.T)].max() > 0
    assert np.array_equal(np.asarray(ph.liquid_fraction), want)
    _assert_summary(ph, 'sync')


# ---- with the moving source and the surface loss on a plate ---------------------------------------------------------------
def test_with_goldak_source_and_surface_loss(mods):
    """24 x 16 x 16 plate, Goldak source strong enough to melt a pool, radiating and convecting surface, 8 steps: the step and
    the stepper's graph against the lagged, corrected loop over the oracle"""
    hip, orc = mods
    import surface_loss_cases as slc
    shape, dx = (24, 16, 16), 5e-4
    dt, theta, Tinf = 2.0 * dx * dx / KAPPA, 0.5, 25.0
    mask = np.ones(shape, dtype=bool)
    mask[:, :, 12:] = False
    mask[8:20, 6:10, 12:14] = True                        # a bead on the plate
    T0 = np.where(mask, 900.0, Tinf)
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    loss = hip.SurfaceLoss(h=15.0, emissivity=0.8)
    src = hip.GoldakSource(power=900.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                           origin=(7 * dx, 8 * dx, 14 * dx), velocity=0.02, travel_axis=0, travel_sign=1, depth_axis=2)
    nst = 8
    go, mato, prmo = orc.Grid3D(*shape, dx, mask), orc.Material(RHO, CP, K), orc.Params(dt, theta)
    T, f = T0, law.f_eq(T0) * mask
    for i in range(nst):
        po = orc.precompute_coeff_packs_unified(go, mato, robin_h=slc.h_fields(loss, T, Tinf))
        po[0].qflux = po[0].qflux + src.sample(go, i * dt + 0.5 * dt) / (RHO * CP)
        T, f = law.correct(orc.adi_step_numba_coeff(T, go, mato, prmo, po, Tinf=Tinf), f, mask, None, CP)
    assert f.max() == 1.0 and ((f > 0) & (f < 1)).any()                       # a pool with a mushy rim
    grid, mat, prm = hip.Grid3D(*shape, dx, mask), hip.Material(RHO, CP, K), hip.Params(dt, theta)
    lp = hip.LossPacks(grid, mat, loss, Tinf)
    ph = hip.PhaseField(grid, mat, law, T=hip.to_device(T0))
    cur = hip.to_device(T0)
    for i in range(nst):
        cur = hip.adi_step_numba_coeff(cur, grid, mat, prm, lp.packs, Tinf=Tinf, S=src, t=i * dt, surface_loss=lp, phase=ph)
    bar_f = 1e-10 * float(np.abs(T).max()) / 50.0
    eT, ef = rel_linf(np.asarray(cur), T), float(np.abs(np.asarray(ph.liquid_fraction) - f).max())
    print('step by step: T rel L-inf %.3e  |df| %.3e (bar %.3e)' % (eT, ef, bar_f))
    assert eT <= 1e-10 and ef <= bar_f
    _assert_summary(ph, 'steps')
    ph.seed(hip.to_device(T0))
    st = hip.StagedStepper(grid, mat, prm, lp.packs, Tinf, source=src, surface_loss=lp, phase=ph)
    got = np.asarray(st.run(hip.to_device(T0), nst, t0=0.0))
    eT, ef = rel_linf(got, T), float(np.abs(np.asarray(ph.liquid_fraction) - f).max())
    assert eT <= 1e-10 and ef <= bar_f
    _assert_summary(ph, 'graph')


# ---- the Stefan problem -----------------------------------------------------------------------------------------------------
def test_stefan_front_on_the_device(mods):
    """4 x 4 lines of 300 cells, the sides adiabatic (tests/test_phase_cpu.py has the one-line run and the figures): the front
    within one cell of Neumann's solution at every quarter of the run after the first, T within 1e-10 of the CPU run"""
    hip, orc = mods
    s = pc.STEFAN
    law = hip.PhaseChange(s['latent'], s['T_melt'] - s['half_range'], s['T_melt'] + s['half_range'])
    lam = pc.stefan_lambda()
    shape, mask, T0, dm, dv, dt = pc.stefan_setup(4)
    go, mato, prmo = orc.Grid3D(*shape, s['dx'], mask), orc.Material(RHO, CP, K), orc.Params(dt, s['theta'])
    po = orc.precompute_coeff_packs_unified(go, mato, dir_mask=dm, dir_value=dv)
    grid, mat, prm = hip.Grid3D(*shape, s['dx'], mask), hip.Material(RHO, CP, K), hip.Params(dt, s['theta'])
    packs = hip.precompute_coeff_packs_unified(grid, mat, dir_mask=dm, dir_value=dv)
    ph = hip.PhaseField(grid, mat, law, T=hip.to_device(T0))
    st = hip.StagedStepper(grid, mat, prm, packs, 0.0, phase=ph)
    T, f = T0, law.f_eq(T0) * mask
    cur = hip.to_device(T0)
    quarter = s['nsteps'] // 4
    for q in range(4):
        for _ in range(quarter):
            T, f = law.correct(orc.adi_step_numba_coeff(T, go, mato, prmo, po, Tinf=0.0), f, mask, dm, CP)
        cur = st.run(cur, quarter)
        gf = np.asarray(ph.liquid_fraction)
        eT, ef = rel_linf(np.asarray(cur), T), float(np.abs(gf - f).max())
        errs = [pc.stefan_front_error(gf[i, j], (q + 1) * quarter, dt, lam) for i in range(4) for j in range(4)]
        print('after %d steps: T rel L-inf %.3e  |df| %.3e  front error %.3f cells' % ((q + 1) * quarter, eT, ef, max(errs)))
        assert eT <= 1e-10 and ef <= 1e-10 * s['T_wall'] / (2.0 * s['half_range'])
        assert max(errs) <= 1.0
    assert st.captures == 1
    _assert_summary(ph, 'stefan')


# ---- the deposition loops -----------------------------------------------------------------------------------------------
def test_run_single_track_with_phase_change(mods):
    """waam.run_single_track on the small plate of the single-track tests: columns of 20 sub-steps (graph path) and, with a
    larger dt, of 4 (step by step), with the moving source, with and without the surface loss, against the column loop written
    here over the oracle"""
    hip, orc = mods
    import surface_loss_cases as slc
    from adi_thermal_fields_amd import waam
    shape, dx = (10, 9, 8), 1e-3
    plate = np.zeros(shape, dtype=bool)
    plate[:, :, :4] = True
    box = (3, 7, 4, 7, 3)                               # x0, x1, z0, z1, columns
    Tinf, T_track, theta, t_step, h = 25.0, 1500.0, 0.5, 0.4, 10.0
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    loss = hip.SurfaceLoss(h=h, emissivity=0.8)
    src0 = hip.GoldakSource(power=300.0, eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
    for dt, with_loss in ((0.02, False), (0.1, True), (0.02, True)):
        got, got_f = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), h, Tinf, T_track, theta, dt, t_step,
                                           heat_source=src0, surface_loss=loss if with_loss else None, phase_change=law)
        x0, x1, z0, z1, ncol = box
        mask = plate.copy()
        grid, mat = orc.Grid3D(*shape, dx, mask), orc.Material(RHO, CP, K)
        T = np.full(shape, Tinf)
        f = np.zeros(shape)
        n_sub = max(1, int(math.ceil(t_step / dt)))
        prm = orc.Params(t_step / n_sub, theta)
        for yi in range(ncol):
            mask[x0:x1, yi:yi + 1, z0:z1] = True
            grid.mask = mask.copy()
            T[x0:x1, yi:yi + 1, z0:z1] = T_track
            f[x0:x1, yi:yi + 1, z0:z1] = law.f_eq(np.float64(T_track))
            src = waam.track_source(src0, box, dx, yi, t_step)
            for i in range(n_sub):
                rh = slc.h_fields(loss, T, Tinf) if with_loss else {fc: h for fc in pc.FACES}
                packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=rh)
                packs[0].qflux = packs[0].qflux + src.sample(grid, i * prm.dt + 0.5 * prm.dt) / (RHO * CP)
                T, f = law.correct(orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf), f, mask, None, CP)
        eT, ef = rel_linf(got, T), float(np.abs(got_f - f).max())
        print('run_single_track dt %.3g loss %s: %d sub-steps per column, T rel L-inf %.3e, |df| %.3e, max f %.3f'
              % (dt, with_loss, n_sub, eT, ef, f.max()))
        assert (n_sub >= waam.GRAPH_MIN_NSUB) == (dt == 0.02)
        assert eT <= 1e-10 and ef <= 1e-10 * T_track / 50.0, (dt, with_loss, eT, ef)
    assert got_f.max() > 0.0                              # the last column is still freezing
    # the latent heat is at work: the run without it differs
    cold = waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), h, Tinf, T_track, theta, 0.02, t_step, heat_source=src0,
                                 surface_loss=loss)
    assert isinstance(cold, np.ndarray) and rel_linf(cold, T) > 1e-3
    with pytest.raises(ValueError, match='device loop'):
        waam.run_single_track(hip, plate, box, dx, (RHO, CP, K), h, Tinf, T_track, theta, 0.1, t_step, device_resident=False,
                              phase_change=law)


def test_run_layer_birth_with_phase_change(mods):
    """waam.run_layer_birth on a 12 x 10 x 14 head born at 1500 degrees, cfl chosen so that the last segment takes the graph
    path and the others the step-by-step one, against the same event loop written here over the oracle"""
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    shape, dx = (12, 10, 14), 1e-3
    full = waam.synthetic_head_mask(*shape)
    layers = waam.plan_layers(full, 2)
    tb = waam.birth_times(full, layers, dx, bead_width=4e-3, scan_speed=8e-3)
    t_out = [tb[-1] + 6.0 * (tb[-1] - tb[-2])]
    Tinf, Ts, theta, cfl, h = 25.0, 1500.0, 0.5, 2.0, 40.0
    law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
    dt_cap = cfl * dx * dx / KAPPA
    nsubs = [max(1, int(math.ceil(a / dt_cap))) for w, a in waam.layer_birth_schedule(tb, t_out) if w == 'advance']
    assert max(nsubs) >= waam.GRAPH_MIN_NSUB and min(nsubs) < waam.GRAPH_MIN_NSUB, nsubs
    got, nsteps, got_f = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), h, Tinf, Ts, theta, cfl, layers, tb, t_out,
                                              phase_change=law)
    mask = np.zeros(shape, dtype=bool)
    grid, mat = orc.Grid3D(*shape, dx, mask), orc.Material(RHO, CP, K)
    T, f = np.full(shape, Tinf), np.zeros(shape)
    want_steps, f_peak = 0, 0.0
    for what, arg in waam.layer_birth_schedule(tb, t_out):
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = orc.Params(max(arg / nsub, 1e-15), theta)
            packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h={fc: h for fc in pc.FACES})
            for _ in range(nsub):
                T, f = law.correct(orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf), f, mask, None, CP)
                f_peak = max(f_peak, float(f.max()))
            want_steps += nsub
        elif what == 'birth':
            ks, ke = layers[arg]
            born = np.zeros(shape, dtype=bool)
            born[:, :, ks:ke + 1] = full[:, :, ks:ke + 1]
            T[born & ~mask] = Ts
            f[born & ~mask] = law.f_eq(np.float64(Ts))
            mask |= born
            grid.mask = mask.copy()
    assert nsteps == want_steps and f_peak > 0.0
    eT, ef = rel_linf(got, T), float(np.abs(got_f - f).max())
    print('run_layer_birth with latent heat: %d steps, T rel L-inf %.3e, |df| %.3e' % (nsteps, eT, ef))
    assert eT <= 1e-10 and ef <= 1e-10 * Ts / 50.0
    plain, _ = waam.run_layer_birth(hip, full, dx, (RHO, CP, K), h, Tinf, Ts, theta, cfl, layers, tb, t_out)
    assert rel_linf(plain, T) > 1e-3
    with pytest.raises(ValueError, match='device loop'):
        waam.run_layer_birth(hip, full, dx, (RHO, CP, K), h, Tinf, Ts, theta, cfl, layers, tb, t_out, phase_change=law,
                             device_loop=False)
