"""GPU: the moving Goldak source on the slab decomposition (SlabStepper(source=...), set_source, step(t=)), several ranks inside
one process on one GPU (dist_slab.LocalComm, one thread per rank), against the single-domain HIP step with the same source
(adi_step_numba_coeff(..., S=src, t=n dt)) in every axis-0 form, and once against the pinned oracle with the source folded
into the axis-0 qflux."""
import threading

import numpy as np
import pytest

from helpers import rel_linf

pytestmark = pytest.mark.gpu

DX = 1e-4
MAT = dict(rho=7800.0, cp=490.0, k=54.0)
ALPHA = 54.0 / (7800.0 * 490.0)


def _ranks(world, fn):
    """fn(rank, comm) on `world` threads over LocalComm -> list of results"""
    import torch
    from adi_thermal_fields_amd import dist_slab
    comms = dist_slab.LocalComm.make(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            out[rank] = fn(rank, comms[rank])
        except Exception as e:   # surface the failure and release the other ranks
            errs.append(e)
            comms[rank].sh.barrier.abort()
    ths = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=180)
    if errs:
        raise errs[0]
    return out


def _case(shape, cfl, kind='solid', seed=0):
    rng = np.random.default_rng(seed)
    mask = np.ones(shape, bool)
    dm = dv = None
    neumann, robin = None, 500.0
    if kind == 'holes':
        mask = rng.random(shape) > 0.05
        dm = (rng.random(shape) < 0.01) & mask
        dv = rng.uniform(300.0, 400.0, shape)
        neumann = {'x-': 4e5, 'z-': 1e4}
        robin = {'x+': 80.0, 'y-': rng.uniform(100.0, 600.0, shape), 'z+': 350.0}
    elif kind == 'ellipsoid':
        g = np.meshgrid(*[(np.arange(s) + 0.5) / s - 0.5 for s in shape], indexing='ij')
        mask = (g[0] / 0.49) ** 2 + (g[1] / 0.46) ** 2 + (g[2] / 0.47) ** 2 <= 1.0
        neumann = {'x-': 3e5, 'y+': 2e5}
    elif kind == 'robin_field':
        neumann = {'x-': 3e5, 'x+': 1e5}
        robin = rng.uniform(100.0, 600.0, shape)
    return dict(shape=shape, mask=mask, dir_mask=dm, dir_value=dv, neumann=neumann, robin_h=robin, Tinf=20.0, theta=0.5,
                dt=cfl * DX * DX / ALPHA, T0=rng.uniform(20.0, 1200.0, shape))


def _source(c, x0, vx=0.0, big=False, **kw):
    """travelling along axis 0 from global x0 (metres), depth along axis 2 from the top of the box"""
    nx, ny, nz = c['shape']
    L = 50.0 * DX if big else None
    d = dict(power=60.0, eta=0.8, a=L or 3.0 * DX, b=L or 2.5 * DX, c_f=L or 3.0 * DX, c_r=L or 6.0 * DX, f_f=0.6,
             origin=(x0, 0.45 * ny * DX, 0.8 * nz * DX), velocity=vx, travel_axis=0, travel_sign=1, depth_axis=2)
    d.update(kw)
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip.GoldakSource(**d)


def _reference(c, src, nsteps, t0=0.0):
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    g = hip.Grid3D(*c['shape'], DX, c['mask'])
    mat, prm = hip.Material(**MAT), hip.Params(c['dt'], c['theta'])
    packs = hip.precompute_coeff_packs_unified(g, mat, dir_mask=c['dir_mask'], dir_value=c['dir_value'],
                                               neumann=c['neumann'], robin_h=c['robin_h'])
    T = np.array(c['T0'])
    for n in range(nsteps):
        T = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=c['Tinf'], S=src, t=t0 + n * c['dt'])
    return np.asarray(T)


def _stepper(c, sizes, rank, comm, opts, src):
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import dist_slab
    i0 = sum(sizes[:rank]); i1 = i0 + sizes[rank]

    def loc(a):
        return a if (a is None or np.isscalar(a)) else np.asarray(a)[i0:i1]
    neumann = None if c['neumann'] is None else {f: loc(v) for f, v in c['neumann'].items()}
    robin = {f: loc(v) for f, v in c['robin_h'].items()} if isinstance(c['robin_h'], dict) else loc(c['robin_h'])
    st = dist_slab.SlabStepper(c['mask'][i0:i1], DX, hip.Material(**MAT), hip.Params(c['dt'], c['theta']), c['Tinf'],
                               dir_mask=loc(c['dir_mask']), dir_value=loc(c['dir_value']), neumann=neumann, robin_h=robin,
                               comm=comm, source=src)
    st._allow_fused = bool(opts.get('allow_fused', True))
    st._allow_window = bool(opts.get('allow_window', True))
    st._allow_deferred = bool(opts.get('allow_deferred', True))
    st._allow_deferred_lines = bool(opts.get('allow_deferred_lines', False))
    st._deferred_lines_cost_ratio = float('inf')
    return st, i0, i1


def _run(c, sizes, nsteps, src, opts=None, t0=0.0):
    """-> (whole field, set of axis0 modes, per-rank plans)"""
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    o = opts or {}

    def fn(rank, comm):
        st, i0, i1 = _stepper(c, sizes, rank, comm, o, src)
        T = hip.to_device(np.ascontiguousarray(c['T0'][i0:i1]))
        for n in range(nsteps):
            if o.get('quick') and n in (1, 2):
                st.set_mask(c['mask'][i0:i1])          # a birth loop re-sets the mask between steps
            T = st.step(T, prefetch_halo=bool(o.get('prefetch', True)) and n + 1 < nsteps, t=t0 + n * c['dt'])
        return T.get(), st.axis0_mode, st._a0
    res = _ranks(len(sizes), fn)
    return np.concatenate([r[0] for r in res], axis=0), {r[1] for r in res}, [r[2] for r in res]


def _check(c, sizes, nsteps, src, mode, opts=None, tol=1e-12):
    got, modes, plans = _run(c, sizes, nsteps, src, opts)
    if mode is not None:
        assert modes == {mode}, modes
    want = _reference(c, src, nsteps)
    err = rel_linf(got, want)
    assert err <= tol, (mode, err)
    plain = _reference(c, None, nsteps)
    assert rel_linf(want, plain) > 1e-6                  # the source did something
    return got, plans


# --- the deferred family: superposition after the local sweep 0 ---------------------------------------------------------
@pytest.mark.parametrize('sizes,fused', [([64, 64], True), ([64, 64], False), ([32] * 4, True), ([32] * 4, False)])
def test_deferred_source_crosses_a_slab_boundary(sizes, fused):
    """all-solid box; the source travels along the sharded axis across the boundary at plane 64 within the run (a dt whose
    weights decay within the slab: cfl 3 on 64 planes, 0.5 on 32)"""
    c = _case((128, 16, 32), 3.0 if sizes[0] == 64 else 0.5, 'robin_field', seed=1)
    nsteps = 5
    src = _source(c, 58.0 * DX, vx=12.0 * DX / (nsteps * c['dt']))
    _, plans = _check(c, sizes, nsteps, src, 'deferred', dict(allow_fused=fused))
    assert all(p['fused'] == fused for p in plans)


def test_deferred_exact_thin_slabs():
    c = _case((64, 16, 32), 200.0, 'robin_field', seed=2)
    src = _source(c, 30.0 * DX, vx=6.0 * DX / (4 * c['dt']))
    _check(c, [16] * 4, 4, src, 'deferred_exact')


def test_deferred_lines_curved_solid():
    c = _case((256, 48, 64), 0.3, 'ellipsoid', seed=3)
    src = _source(c, 120.0 * DX, vx=16.0 * DX / (4 * c['dt']), origin=(120.0 * DX, 24.0 * DX, 40.0 * DX))
    _check(c, [64] * 4, 4, src, 'deferred_lines', dict(allow_deferred_lines=True))


# --- the two-pass forms: the source in R0 ----------------------------------------------------------------------------------
@pytest.mark.parametrize('cfl,opts,mode', [(0.1, {}, 'window'), (3.0, {}, 'slab'), (0.1, dict(allow_window=False), 'slab'),
                                           (300.0, {}, 'exact')])
def test_two_pass_forms_with_holes_dirichlet_robin_neumann(cfl, opts, mode):
    c = _case((256, 10, 40), cfl, 'holes', seed=4)
    src = _source(c, 60.0 * DX, vx=8.0 * DX / (4 * c['dt']), origin=(60.0 * DX, 5.0 * DX, 30.0 * DX))
    _, plans = _check(c, [64] * 4, 4, src, mode, dict(opts, allow_deferred=False))
    assert not any(p['fused'] or p['dots'] for p in plans), [(p['fused'], p['dots']) for p in plans]


def test_dots_eligible_solid_runs_without_dots():
    """an all-solid box takes the dot-product pass A without a source; with one, R0 must be read as stored"""
    c = _case((128, 16, 32), 3.0, 'robin_field', seed=5)
    got0, modes0, plans0 = _run(c, [64, 64], 2, None, dict(allow_deferred=False))
    assert modes0 == {'slab'} and all(p['dots'] for p in plans0)
    src = _source(c, 62.0 * DX)
    _, plans = _check(c, [64, 64], 3, src, 'slab', dict(allow_deferred=False))
    assert not any(p['dots'] or p['fused'] for p in plans)


def test_quick_plan_after_two_set_mask_calls():
    c = _case((256, 10, 40), 3.0, 'holes', seed=6)
    src = _source(c, 64.0 * DX, vx=4.0 * DX / (4 * c['dt']), origin=(64.0 * DX, 5.0 * DX, 30.0 * DX))
    _, plans = _check(c, [64] * 4, 4, src, 'slab', dict(allow_deferred=False, quick=True))
    assert all(p.get('quick') and not p['fused'] and not p['dots'] for p in plans)


# --- geometries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deferred', [True, False])
def test_source_centred_on_a_boundary_plane(deferred):
    c = _case((128, 16, 32), 3.0, 'robin_field', seed=7)
    src = _source(c, 64.0 * DX)                           # the face between global planes 63 and 64: the slab boundary
    _check(c, [64, 64], 3, src, 'deferred' if deferred else 'slab', dict(allow_deferred=deferred))


@pytest.mark.parametrize('deferred', [True, False])
def test_support_on_one_rank_heats_the_neighbour(deferred):
    c = _case((128, 16, 32), 3.0, 'robin_field', seed=8)
    src = _source(c, 50.0 * DX)                           # planes 28 .. 60 (front 11 planes, rear 22): rank 0 of [64, 64] only
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip

    def fn(rank, comm):
        st, i0, i1 = _stepper(c, [64, 64], rank, comm, dict(allow_deferred=deferred), src)
        meets = st._source_meets(src, 0.0, c['dt'], st._plane_origin())
        T = st.step(hip.to_device(np.ascontiguousarray(c['T0'][i0:i1])), t=0.0)
        return T.get(), meets, st.axis0_mode
    res = _ranks(2, fn)
    assert [r[1] for r in res] == [True, False]
    assert {r[2] for r in res} == {'deferred' if deferred else 'slab'}
    got = np.concatenate([r[0] for r in res], axis=0)
    want = _reference(c, src, 1)
    assert rel_linf(got, want) <= 1e-12
    plain = _reference(c, None, 1)
    assert np.abs(got[64:] - plain[64:]).max() > 1e-6    # the heat reaches the rank that launched nothing


@pytest.mark.parametrize('deferred', [True, False])
def test_support_wider_than_the_grid(deferred):
    c = _case((128, 16, 32), 3.0, 'robin_field', seed=9)
    src = _source(c, 70.0 * DX, big=True)
    _check(c, [64, 64], 2, src, 'deferred' if deferred else 'slab', dict(allow_deferred=deferred))


@pytest.mark.parametrize('deferred', [True, False])
def test_padded_planes_and_uneven_slabs(deferred):
    """planes of 24 x 40 are padded (adi_recommended_dims); slabs of 64, 62, 64 planes"""
    c = _case((190, 24, 40), 1.0, 'robin_field', seed=10)
    src = _source(c, 60.0 * DX, vx=10.0 * DX / (4 * c['dt']), origin=(60.0 * DX, 20.0 * DX, 35.0 * DX))
    _check(c, [64, 62, 64], 4, src, 'deferred' if deferred else None, dict(allow_deferred=deferred))


def test_one_rank():
    c = _case((64, 16, 32), 3.0, 'holes', seed=11)
    src = _source(c, 30.0 * DX, vx=4.0 * DX / (3 * c['dt']), origin=(30.0 * DX, 8.0 * DX, 25.0 * DX))
    _check(c, [64], 3, src, None)


def test_against_the_oracle_with_the_source_in_qflux():
    from oracle import adi_oracle as orc
    c = _case((64, 12, 20), 0.5, 'holes', seed=12)
    src = _source(c, 28.0 * DX, vx=8.0 * DX / (3 * c['dt']), origin=(28.0 * DX, 6.0 * DX, 15.0 * DX))
    got, _, _ = _run(c, [32, 32], 3, src, dict(allow_deferred=False))
    g = orc.Grid3D(*c['shape'], DX, c['mask'])
    mat, prm = orc.Material(**MAT), orc.Params(c['dt'], c['theta'])
    T = np.array(c['T0'])
    for n in range(3):
        packs = orc.precompute_coeff_packs_unified(g, mat, dir_mask=c['dir_mask'], dir_value=c['dir_value'],
                                                   neumann=c['neumann'], robin_h=c['robin_h'])
        packs[0].qflux = packs[0].qflux + src.sample(g, (n + 0.5) * c['dt']) / (MAT['rho'] * MAT['cp'])
        T = orc.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=c['Tinf'])
    assert rel_linf(got, T) <= 1e-10, rel_linf(got, T)


# --- nothing changes without a source; a moving source plans once ----------------------------------------------------------
@pytest.mark.parametrize('deferred', [True, False])
def test_without_a_source_nothing_changes(deferred):
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    c = _case((128, 16, 32), 3.0, 'robin_field', seed=13)
    src = _source(c, 60.0 * DX)
    o = dict(allow_deferred=deferred)
    never, _, _ = _run(c, [64, 64], 3, None, dict(o, prefetch=False))

    def detached(rank, comm):                             # attached at construction, detached before the first step
        st, i0, i1 = _stepper(c, [64, 64], rank, comm, o, src)
        st.set_source(None)
        T = hip.to_device(np.ascontiguousarray(c['T0'][i0:i1]))
        for n in range(3):
            T = st.step(T)
        return T.get()
    np.testing.assert_array_equal(np.concatenate(_ranks(2, detached), axis=0), never)

    def after(rank, comm):                                # two steps with the source, then without it
        st, i0, i1 = _stepper(c, [64, 64], rank, comm, o, src)
        T = hip.to_device(np.ascontiguousarray(c['T0'][i0:i1]))
        for n in range(2):
            T = st.step(T, t=n * c['dt'])
        mid = T.get()
        st.set_source(None)
        for n in range(2):
            T = st.step(T)
        return mid, T.get()
    res = _ranks(2, after)
    mid = np.concatenate([r[0] for r in res], axis=0)
    got = np.concatenate([r[1] for r in res], axis=0)
    c2 = dict(c, T0=mid)
    want, _, _ = _run(c2, [64, 64], 2, None, dict(o, prefetch=False))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('deferred', [True, False])
def test_moving_source_plans_once(deferred):
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    c = _case((128, 16, 32), 3.0, 'robin_field', seed=14)
    src = _source(c, 40.0 * DX, vx=40.0 * DX / (10 * c['dt']))

    def fn(rank, comm):
        st, i0, i1 = _stepper(c, [64, 64], rank, comm, dict(allow_deferred=deferred), src)
        T = hip.to_device(np.ascontiguousarray(c['T0'][i0:i1]))
        T = st.step(T, t=0.0)
        plan, steps0 = st._a0, st._plan_steps
        for n in range(1, 10):
            T = st.step(T, t=n * c['dt'])
        return plan is st._a0, st._plan_steps - steps0, T.get()
    res = _ranks(2, fn)
    assert all(r[0] and r[1] == 9 for r in res), [(r[0], r[1]) for r in res]
    got = np.concatenate([r[2] for r in res], axis=0)
    assert rel_linf(got, _reference(c, src, 10)) <= 1e-12


# --- the single-track driver -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 3])
def test_single_track_slab_with_heat_source(world):
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    from adi_thermal_fields_amd.dist_slab import split_planes
    nx, ny, nz, dx = 16, 20, 14, 2.5e-4
    plate = np.zeros((nx, ny, nz), dtype=bool)
    plate[:, :, :6] = True
    box = (6, 10, 6, 9, 6)
    h, Tinf, T_track, theta, dt, t_step = 20.0, 300.0, 1800.0, 0.5, 0.02, 0.05
    src = hip.GoldakSource(600.0, 0.7, 5e-4, 4e-4, 5e-4, 1e-3)
    rho, cp, k = MAT['rho'], MAT['cp'], MAT['k']
    want = waam.run_single_track(hip, plate, box, dx, (rho, cp, k), h, Tinf, T_track, theta, dt, t_step, heat_source=src)
    sizes = split_planes(nx, world)

    def fn(rank, comm):
        i0 = sum(sizes[:rank])
        return waam.run_single_track_slab(comm, i0, i0 + sizes[rank], plate, box, dx, hip.Material(rho, cp, k), hip.Params,
                                          h, Tinf, T_track, theta, dt, t_step, heat_source=src)
    got = np.concatenate(_ranks(world, fn), axis=0)
    assert rel_linf(got, want) <= 1e-12, rel_linf(got, want)
    plain = waam.run_single_track(hip, plate, box, dx, (rho, cp, k), h, Tinf, T_track, theta, dt, t_step)
    assert got.max() > np.asarray(plain).max() + 1.0
