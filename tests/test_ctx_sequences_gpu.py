"""GPU: the stateful layers above the Cartesian kernels driven through SEQUENCES of calls -- the context half of the C ABI
(adi_ctx_*, raw ctypes as a non-Python consumer of include/adi_hip.h would drive it), and PromiseLedger / StagedStepper /
HipEngine of the Python hosts -- with dt and theta changing under one pack set.  Every number is compared with oracle.adi_oracle stepped
through the same sequence, at the project's bar rel_linf <= 1e-10.

Why: the no-fallback promise (bit 2 of `sparse`) is learnt from the unit queue of a sweep, and a sweep with
theta * gam < kMixedMinTg = 1e-9 (a vanishing time step, theta = 0 included) runs no FAST kernel, so its queue reads "empty"
whatever the mask.  A promise learnt there and used at an ordinary dt leaves every queued unit (Dirichlet cells, segments
with three or more runs, ...) unsolved."""
import ctypes

import numpy as np
import pytest

from helpers import rel_linf

pytestmark = pytest.mark.gpu

TOL = 1e-10                      # the bar of test_hip_ctx_api.py / test_hip_parity.py (BASELINE.json north_star)
RHO, CP, K = 7800.0, 490.0, 54.0         # steel
ALPHA = K / (RHO * CP)
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
GAM_TINY = 1e-10                 # theta * gam <= 1e-10 < kMixedMinTg: GENERAL kernels only
I6, D6, P6 = ctypes.c_int * 6, ctypes.c_double * 6, ctypes.c_void_p * 6
NULL_FIELD = 'null'              # face spec: ADI_FACE_FIELD with a NULL pointer


def dt_of(gam, dx):
    return gam * dx * dx / ALPHA


def _faces(spec):
    """6 entries None | float | ndarray | NULL_FIELD -> (modes, scalars, pointers, arrays kept alive)"""
    modes, scal, ptrs, keep = I6(), D6(), P6(), []
    for i, v in enumerate(spec):
        if v is None:
            modes[i] = 0
        elif isinstance(v, str):
            modes[i] = 2                                   # FIELD, pointer left NULL
        elif np.isscalar(v):
            modes[i], scal[i] = 1, float(v)
        else:
            a = np.ascontiguousarray(v, dtype=np.float64)
            keep.append(a)
            modes[i], ptrs[i] = 2, a.ctypes.data
    return modes, scal, ptrs, keep


class Ctx:
    """adi_ctx_* through raw ctypes"""

    def __init__(self, shape, dx):
        from adi_thermal_fields_amd import _lib
        self.L, self.lib, self.shape = _lib, _lib.lib, tuple(shape)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.adi_ctx_create(*shape, dx, 0, ctypes.byref(self.h)))

    def close(self):
        self.lib.adi_ctx_destroy(self.h)

    def set_mask(self, mask):
        m8 = np.ascontiguousarray(mask, dtype=np.bool_).view(np.uint8)
        self.L.check(self.lib.adi_ctx_set_mask(self.h, m8.ctypes.data))

    def build(self, h, q, dm=None, dv=None):
        hm, hs, hf, k1 = _faces(h)
        qm, qs, qf, k2 = _faces(q)
        d8 = None if dm is None else np.ascontiguousarray(dm, dtype=np.bool_).view(np.uint8)
        dvv = None if dv is None else np.ascontiguousarray(dv, dtype=np.float64)
        self.L.check(self.lib.adi_ctx_build_coeffs(self.h, RHO, CP, hm, hs, hf, qm, qs, qf,
                                                   None if d8 is None else d8.ctypes.data,
                                                   None if dvv is None else dvv.ctypes.data))

    def upload(self, T):
        T = np.ascontiguousarray(T, dtype=np.float64)
        self.L.check(self.lib.adi_ctx_upload_T(self.h, T.ctypes.data))

    def step(self, dt, theta, Tinf, nsteps):
        self.L.check(self.lib.adi_ctx_step(self.h, RHO, CP, K, dt, theta, Tinf, nsteps))

    def download(self):
        T = np.empty(self.shape)
        self.L.check(self.lib.adi_ctx_download_T(self.h, T.ctypes.data))
        return T

    def pack(self, axis):
        co, qf = np.empty(self.shape), np.empty(self.shape)
        self.L.check(self.lib.adi_ctx_download_pack(self.h, axis, co.ctypes.data, qf.ctypes.data))
        return co, qf


def oracle_packs(grid, h, q, dm, dv):
    """the oracle's packs for the same face specs (a face without h is h = 0 there: the same coefficient)"""
    from oracle import adi_oracle as orc
    rh = None if all(v is None for v in h) else {f: (0.0 if v is None else v) for f, v in zip(FACES, h)}
    nq = {f: v for f, v in zip(FACES, q) if v is not None}
    return orc.precompute_coeff_packs_unified(grid, orc.Material(RHO, CP, K), dir_mask=dm, dir_value=dv,
                                              neumann=nq or None, robin_h=rh)


def oracle_steps(T, grid, packs, dt, theta, Tinf, nsteps):
    from oracle import adi_oracle as orc
    mat, prm = orc.Material(RHO, CP, K), orc.Params(dt, theta)
    for _ in range(nsteps):
        T = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
    return T


# ---------------------------------------------------------------------------------------------------------------------
# (a), (b): the promise across a change of time step
# ---------------------------------------------------------------------------------------------------------------------
SHAPE_P = (256, 16, 32)          # the shape of the existing promise tests: FAST kernels on axes 0 and 2
DX = 1e-3


def promise_config(name):
    """(mask, dir_mask, dir_value): two configurations whose FAST kernels queue units at an ordinary step"""
    if name == 'dirichlet_plane':
        dm = np.zeros(SHAPE_P, bool)
        dm[:, 0, :] = True
        return np.ones(SHAPE_P, bool), dm, np.full(SHAPE_P, 55.0)
    rng = np.random.default_rng(11)
    rng.uniform(20.0, 900.0, SHAPE_P)                      # (the draws of test_ctx_learns_the_no_fallback_promise)
    return rng.random(SHAPE_P) > 0.05, None, None


def queued_counts(name, gam, theta):
    """adi_step_queued on torch buffers for the same mask and packs -> the three queue counts"""
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import _lib
    mask, dm, dv = promise_config(name)
    grid = hip.Grid3D(*SHAPE_P, DX, mask)
    packs = hip.precompute_coeff_packs_unified(grid, hip.Material(RHO, CP, K), robin_h=300.0, dir_mask=dm, dir_value=dv)
    L = grid.layout
    T = hip.to_device(np.random.default_rng(3).uniform(20.0, 900.0, SHAPE_P)).t
    out, ta, tb = L.empty(), L.empty(), L.empty()
    _, work, wb = grid.scratch(2)
    work.fill_(255)
    q = (ctypes.c_uint * 3)(7, 7, 7)
    coeff = _lib.ptr_array([p.d_coeff.data_ptr() for p in packs])
    qflux = _lib.ptr_array([None, None, None])
    p0 = packs[0]
    _lib.check(_lib.lib.adi_step_queued(hip._p(T), hip._p(out), hip._p(ta), hip._p(tb), hip._p(grid.d_flags), coeff,
                                        hip._p(p0.d_dir_mask), hip._p(p0.d_dir_val), qflux, p0.variant,
                                        hip._sparse_arg(grid, p0, False), *L.pd, DX, RHO, CP, K, dt_of(gam, DX), theta, 20.0,
                                        None, hip._p(work), wb, hip._stream(), ctypes.cast(q, ctypes.c_void_p)))
    torch.cuda.synchronize()
    return list(q)


@pytest.mark.parametrize('order', ['vanishing_first', 'ordinary_first'])
@pytest.mark.parametrize('theta_v', [0.5, 0.0])
@pytest.mark.parametrize('name', ['dirichlet_plane', 'holes'])
def test_ctx_promise_is_not_carried_across_the_time_step_gate(name, theta_v, order):
    """One context, one pack set; a step with gam = 1e-10 (theta_v * gam below kMixedMinTg; theta_v = 0: forward Euler, which
    the oracle takes and which stays finite at this dt) before or between steps with gam = 60, a download after every
    call.  The vanishing step launches no FAST kernel and reports three empty queues; at gam = 60 the same mask and packs do
    queue units (both asserted here, so the test cannot pass because nothing was at stake).
    Without the fix, by the code: the vanishing step teaches promise = 1, the first gam = 60 call of 'vanishing_first' runs the FAST
    kernels without queue or fallback and the queued units keep stale scratch; 'ordinary_first' learns "no" first and passes.
    (Figures of the unfixed library on hardware: not measured yet -- the printed rel_linf per call is there for that.)"""
    from oracle import adi_oracle as orc
    q_ord, q_van = queued_counts(name, 60.0, 0.5), queued_counts(name, GAM_TINY, theta_v)
    print('queued at gam=60: %s, at gam=1e-10: %s' % (q_ord, q_van))
    assert any(v > 0 for v in q_ord), q_ord
    assert q_van == [0, 0, 0], q_van
    mask, dm, dv = promise_config(name)
    van, ordi = (dt_of(GAM_TINY, DX), theta_v), (dt_of(60.0, DX), 0.5)
    calls = [van + (1,), ordi + (1,), ordi + (3,)] if order == 'vanishing_first' else [ordi + (1,), van + (1,), ordi + (3,)]
    T0 = np.random.default_rng(5).uniform(20.0, 900.0, SHAPE_P)
    og = orc.Grid3D(*SHAPE_P, DX, mask)
    pk = oracle_packs(og, [300.0] * 6, [None] * 6, dm, dv)
    c = Ctx(SHAPE_P, DX)
    try:
        c.set_mask(mask)
        c.build([300.0] * 6, [None] * 6, dm, dv)
        c.upload(T0)
        want = np.array(T0)
        errs = []
        for dt, theta, n in calls:
            c.step(dt, theta, 20.0, n)
            want = oracle_steps(want, og, pk, dt, theta, 20.0, n)
            assert np.isfinite(want).all()
            errs.append(rel_linf(c.download(), want))
        print('rel_linf per call:', errs)
        assert max(errs) <= TOL, errs
    finally:
        c.close()


def _py_sequence(api, step, T, grid, packs, calls):
    for dt, n in calls:
        prm = api.Params(dt, 0.5)
        for _ in range(n):
            T = step(T, grid, api.Material(RHO, CP, K), prm, packs, Tinf=20.0)
    return T


def test_python_host_promise_is_not_carried_across_the_time_step_gate():
    """The same defect one layer up: the single-domain host keeps its PromiseLedger on the PACK, so every stepper on those packs shares it.
    One Grid3D, a Dirichlet plane (queues at an ordinary step), the queue word of the workspace at 0 as after any sweep that
    queued nothing.  (1) adi_step_hip_coeff: LEARN_AFTER steps at gam = 1e-10, then 3 at gam = 60, same packs.  (2)
    StagedStepper A (gam = 1e-10) through step / run(graph=False) / run(graph=True), then stepper B (gam = 60) on the same
    packs through the same three -- against the oracle, and bit for bit against plain stepping on packs nobody taught.
    Afterwards no entry of p._nofb is True.
    Without the fix, by the code: the vanishing sweeps read the stale 0 and learn True, and the gam = 60 steps leave the Dirichlet
    units unsolved.  (Figures of the unfixed host on hardware: not measured yet; both rel_linf values are printed.)"""
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd._ledger import PromiseLedger
    from oracle import adi_oracle as orc
    mask, dm, dv = promise_config('dirichlet_plane')
    tiny, ordi = dt_of(GAM_TINY, DX), dt_of(60.0, DX)
    T0 = np.random.default_rng(8).uniform(20.0, 900.0, SHAPE_P)
    og = orc.Grid3D(*SHAPE_P, DX, mask)
    opk = orc.precompute_coeff_packs_unified(og, orc.Material(RHO, CP, K), robin_h=300.0, dir_mask=dm, dir_value=dv)
    grid = hip.Grid3D(*SHAPE_P, DX, mask)
    mat = hip.Material(RHO, CP, K)

    def fresh_packs():
        return hip.precompute_coeff_packs_unified(grid, mat, robin_h=300.0, dir_mask=dm, dir_value=dv)

    def zero_queue_word():
        _, work, _ = grid.scratch(2)
        work[:4].zero_()
    # (1) the step function
    n_learn = PromiseLedger.LEARN_AFTER
    calls = [(tiny, n_learn), (ordi, 3)]
    packs = fresh_packs()
    zero_queue_word()
    got = _py_sequence(hip, hip.adi_step_hip_coeff, hip.to_device(T0), grid, packs, calls).get()
    want = _py_sequence(orc, orc.adi_step_numba_coeff, np.array(T0), og, opk, calls)
    e1 = rel_linf(got, want)
    print('adi_step_hip_coeff: rel_linf', e1, [v for p in packs for v in p._nofb.values()])
    assert e1 <= TOL, e1
    assert not any(v is True for p in packs for v in p._nofb.values())
    # (2) two steppers on one pack set
    packs = fresh_packs()
    zero_queue_word()
    T = hip.to_device(T0)
    for dt in (tiny, ordi):
        st = hip.StagedStepper(grid, mat, hip.Params(dt, 0.5), packs, Tinf=20.0)
        T = st.step(T)
        T = st.run(T, 2, graph=False)
        T = st.run(T, 4, graph=True)
    torch.cuda.synchronize()
    got = T.get()
    calls = [(tiny, 7), (ordi, 7)]
    want = _py_sequence(orc, orc.adi_step_numba_coeff, np.array(T0), og, opk, calls)
    e2 = rel_linf(got, want)
    print('StagedStepper: rel_linf', e2, [v for p in packs for v in p._nofb.values()])
    assert e2 <= TOL, e2
    assert not any(v is True for p in packs for v in p._nofb.values())
    plain = _py_sequence(hip, hip.adi_step_hip_coeff, hip.to_device(T0), grid, fresh_packs(), calls).get()
    assert np.array_equal(got, plain)                      # the same kernels, with or without a graph


class _EngineSlab:
    """one slab that is the whole box, on one HipEngine and no communicator: extended arrays with empty halo planes, flags and
    packs from E.build_flags / E.build_packs the way SlabStepper.set_mask builds them, interior views for the sweeps"""

    def __init__(self, E, mask, dm, dv, T0):
        import torch
        import adi_thermal_fields_amd.adi3d_hip_coeff as hip
        nx, ny, nz = mask.shape
        assert E.plane_dims(ny, nz) == (ny, nz)                  # no padded planes at this shape

        def ext(a, fill):
            e = np.full((nx + 2, ny, nz), fill, dtype=a.dtype)
            e[1:-1] = a
            return e
        self.E, self.Lext, self.Li = E, E.layout(nx + 2, ny, nz), E.layout(nx, ny, nz)
        assert self.Li.sx == self.Lext.sx
        d_mask = self.Lext.to_layout(ext(mask, False), torch.uint8)
        flags = E.build_flags(self.Lext, d_mask)
        packs = E.build_packs(self.Lext, d_mask, flags, DX, hip.Material(RHO, CP, K), ext(dm, False), ext(dv, 0.0), None, 300.0)
        self.v, self.fl = packs[0].variant, flags[1:-1]
        self.pk = [tuple(None if t is None else t[1:-1] for t in (p.d_coeff, p.d_dir_mask, p.d_dir_val, p.d_qflux))
                   for p in packs]
        self.keep = (d_mask, flags, packs)
        self.Text = self.Lext.to_layout(ext(T0, 0.0), torch.float64)
        self.out = [self.Lext.empty(zero=True)[1:-1] for _ in range(2)]
        self.zero, self.ones = E.vec(ny * nz), E.vec(nx).fill_(1.0)

    def run(self, form, gam):
        """one call of each entry point of `form` at theta = 0.5 -> the outputs"""
        E, Li, Ti, dt, th = self.E, self.Li, self.Text[1:-1], dt_of(gam, DX), 0.5
        if form == 'sweep':                                      # axis 0 (256 rows: FAST kernel, queue), then axis 1 (16 rows)
            E.sweep(0, self.v, Li, Ti, self.fl, self.pk[0], th, gam, dt, 20.0, self.out[0])
            E.sweep(1, self.v, Li, Ti, self.fl, self.pk[1], th, gam, dt, 20.0, self.out[1])
            return self.out
        if form == 'fused':
            E.sweep0_fused(self.v, Li, self.Text, 1, 0, self.fl, self.pk[0], DX, dt, ALPHA, th, 20.0, self.out[0])
        else:
            E.sweep_corrected(self.v, Li, Ti, self.fl, self.pk[1], th, gam, dt, 20.0, self.out[0], self.zero, self.zero,
                              self.ones)
        return self.out[:1]


def test_slab_engine_promise_is_not_carried_across_the_time_step_gate():
    """The same defect in the other Python host: dist_slab.HipEngine keeps its PromiseLedger on the ENGINE, under keys of data
    pointers.  One engine, the box as one slab, a Dirichlet plane (queues at an ordinary step), the queue word of the engine's
    workspace at 0; LEARN_AFTER calls of E.sweep at gam = 1e-10, then three at gam = 60.  Afterwards no entry of E._nofb is True,
    the last output equals bit for bit that of an engine that never saw the small time step, and it agrees with adi_sweep_axis
    of the single-domain host.  Then the same, bit for bit, for sweep0_fused and for sweep_corrected with zero ulo / uhi.
    Every call of E.sweep(1, ...) is preceded by E.sweep(0, ...) with the same arguments, as in a step: axis 1 of this box has
    16 rows, below the 64 from which a strided FAST kernel exists (strided_plan, csrc/adi_cart_host.hpp), so on its own it
    neither queues anything nor writes the queue word -- nothing would be at stake, and the third call at gam = 60 would read
    back the 0 this test put there.  Along axis 0 (256 rows) the FAST kernel runs and queues the Dirichlet tiles: its entry
    must come out False (asserted), and the read-back of axis 1 then sees that count, as it does inside a step.
    Without the fix, by the code: the vanishing sweeps read the stale 0 and learn True, and the gam = 60 sweeps along axis 0
    leave the queued tiles unsolved.  On an MI355X: every entry False after each form, rel_linf 8.4e-16 (axis 0) and
    2.6e-15 (axis 1) against adi_sweep_axis."""
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import dist_slab
    from adi_thermal_fields_amd._ledger import PromiseLedger
    mask, dm, dv = promise_config('dirichlet_plane')
    T0 = np.random.default_rng(8).uniform(20.0, 900.0, SHAPE_P)
    taught, fresh = (_EngineSlab(dist_slab.HipEngine(), mask, dm, dv, T0) for _ in range(2))
    E = taught.E
    for form in ('sweep', 'fused', 'corrected'):
        E._workspace(taught.Li)[:4].zero_()
        before = dict(E._nofb)
        for _ in range(PromiseLedger.LEARN_AFTER):
            taught.run(form, GAM_TINY)
        assert dict(E._nofb) == before                             # a sweep below the gate does not even count
        for _ in range(3):
            got = taught.run(form, 60.0)
        want = fresh.run(form, 60.0)
        torch.cuda.synchronize()
        print(form, 'E._nofb:', list(E._nofb.values()), 'fresh:', list(fresh.E._nofb.values()))
        assert not any(v is True for v in E._nofb.values())
        for a, b in zip(got, want):
            assert torch.equal(a, b), form
        if form == 'sweep':
            assert [v for k, v in E._nofb.items() if k[1] == 0] == [False]      # axis 0 did queue: something was at stake
            grid = hip.Grid3D(*SHAPE_P, DX, mask)
            mat = hip.Material(RHO, CP, K)
            packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=300.0, dir_mask=dm, dir_value=dv)
            for axis in (0, 1):
                ref = hip.adi_sweep_axis(axis, T0, grid, mat, hip.Params(dt_of(60.0, DX), 0.5), packs[axis], Tinf=20.0)
                e = rel_linf(got[axis].cpu().numpy(), ref)
                print('E.sweep(%d) against adi_sweep_axis: rel_linf' % axis, e)
                assert e <= TOL, (axis, e)


# ---------------------------------------------------------------------------------------------------------------------
# (c): seeded sequence fuzz of the context
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_SHAPES = [(256, 16, 32), (16, 128, 32),     # FAST kernels on a strided axis
               (24, 20, 96),                     # contiguous FAST
               (70, 5, 66),                      # ragged, padded planes
               (1040, 4, 8),                     # the workspace holds c' / d': no queue exists
               (1, 7, 9)]
FUZZ_SEEDS = list(range(12))
GAMS = (1e-10, 0.3, 60.0, 3000.0)


def _mask(rng, shape, kind):
    if kind == 'solid':
        return np.ones(shape, bool)
    if kind in ('holes5', 'holes30'):
        return rng.random(shape) > (0.05 if kind == 'holes5' else 0.30)
    nx, ny, nz = shape                                     # a disk column along axis 0
    j, k = np.meshgrid(np.arange(ny) - (ny - 1) / 2.0, np.arange(nz) - (nz - 1) / 2.0, indexing='ij')
    disk = (j / (0.5 * ny)) ** 2 + (k / (0.5 * nz)) ** 2 <= 0.85
    return np.broadcast_to(disk, shape).copy()


def _face_specs(rng, shape, lo, hi):
    out, tags = [], set()
    for _ in range(6):
        m = int(rng.integers(3))
        tags.add(('NONE', 'SCALAR', 'FIELD')[m])
        out.append(None if m == 0 else (float(rng.uniform(lo, hi)) if m == 1 else rng.uniform(lo, hi, shape)))
    return out, tags


def make_program(seed, base=1000):
    """-> (shape, dx, ops, tags).  A random program of 8 to 12 context operations with every input drawn here; the generator
    tracks the context's state rules and marks the operations that must be refused (`error`).  tags: what the program covers."""
    rng = np.random.default_rng(base + seed)
    shape = FUZZ_SHAPES[seed % len(FUZZ_SHAPES)]
    dx = 1e-3
    n = int(rng.integers(8, 13))
    ops, tags = [], set()
    have_mask = have_packs = have_T = built_once = False
    odd = False                                            # steps since the last upload: odd
    while len(ops) < n:
        i = len(ops)
        if i == n - 1:
            kind = 'download_T'
        elif i == 0:
            kind = rng.choice(['build', 'download_T', 'set_mask'], p=[0.3, 0.3, 0.4])
        elif not have_mask:
            kind = 'set_mask'
        elif not have_packs:
            kind = rng.choice(['build', 'step', 'download_pack', 'build_null'], p=[0.55, 0.15, 0.15, 0.15])
        elif not have_T:
            kind = 'upload'
        elif ops[-1]['op'] == 'step' and rng.random() < 0.7:
            kind = 'download_T'
        else:
            kind = rng.choice(['step', 'download_T', 'download_pack', 'upload', 'set_mask', 'build'],
                              p=[0.5, 0.1, 0.08, 0.12, 0.12, 0.08])
        if kind == 'set_mask':
            mk = str(rng.choice(['solid', 'holes5', 'holes30', 'disk']))
            ops.append(dict(op='set_mask', mask=_mask(rng, shape, mk)))
            tags.add('mask:' + mk)
            have_mask, have_packs = True, False
        elif kind in ('build', 'build_null'):
            h, th = _face_specs(rng, shape, 50.0, 800.0)
            q, tq = _face_specs(rng, shape, -1e5, 2e5)
            tags |= {'h:' + t for t in th} | {'q:' + t for t in tq}
            dk = str(rng.choice(['none', 'plane_null', 'rand5', 'zeros']))
            dm = dv = None
            if dk == 'plane_null':                         # h_dir_val = NULL: the reference's "None means 0"
                dm = np.zeros(shape, bool)
                dm[:, 0, :] = True
            elif dk == 'rand5':
                dm, dv = rng.random(shape) < 0.05, rng.uniform(20.0, 500.0, shape)
            elif dk == 'zeros':                            # selects the no-Dirichlet variant
                dm, dv = np.zeros(shape, bool), rng.uniform(20.0, 500.0, shape)
            err = not have_mask
            if kind == 'build_null':
                (h if rng.random() < 0.5 else q)[int(rng.integers(6))] = NULL_FIELD
                err = True
                tags.add('err:null_field')
            elif err:
                tags.add('err:build_before_mask')
            else:
                tags.add('dir:' + dk)
                have_packs = built_once = True
            ops.append(dict(op='build', h=h, q=q, dm=dm, dv=dv, error=err))
        elif kind == 'upload':
            ops.append(dict(op='upload', T=rng.uniform(20.0, 900.0, shape)))
            if odd:
                tags.add('upload_after_odd_steps')
            have_T, odd = True, False
        elif kind == 'step':
            err = not (have_mask and have_packs and have_T)
            ns = int(rng.integers(4))
            gam, theta = float(rng.choice(GAMS)), float(rng.choice([0.5, 1.0]))
            ops.append(dict(op='step', dt=dt_of(gam, dx), theta=theta, Tinf=float(rng.uniform(0.0, 100.0)), nsteps=ns, error=err))
            if err:
                tags.add('err:step_after_remask' if built_once else 'err:step_before_build')
            else:
                tags |= {'gam:%g' % gam, 'theta:%g' % theta, 'nsteps:%d' % ns}
                odd ^= bool(ns & 1)
        elif kind == 'download_T':
            ops.append(dict(op='download_T', error=not have_T))
            if not have_T:
                tags.add('err:download_before_upload')
        else:
            ops.append(dict(op='download_pack', axis=int(rng.integers(3)), error=not have_packs))
            tags.add('download_pack' if have_packs else ('err:pack_after_remask' if built_once else 'err:pack_before_build'))
    return shape, dx, ops, tags


def run_oracle(shape, dx, ops):
    """-> per operation: the expected field (download_T), (coeff, qflux) (download_pack) or None"""
    from oracle import adi_oracle as orc
    grid = packs = T = None
    out = []
    for o in ops:
        res = None
        if o.get('error'):
            pass
        elif o['op'] == 'set_mask':
            grid = orc.Grid3D(*shape, dx, o['mask'])
        elif o['op'] == 'build':
            packs = oracle_packs(grid, o['h'], o['q'], o['dm'], o['dv'])
        elif o['op'] == 'upload':
            T = np.array(o['T'])
        elif o['op'] == 'step':
            T = oracle_steps(T, grid, packs, o['dt'], o['theta'], o['Tinf'], o['nsteps'])
        elif o['op'] == 'download_T':
            res = np.array(T)
        else:
            res = (packs[o['axis']].coeff, packs[o['axis']].qflux)
        out.append(res)
    return out


def run_ctx(c, ops, want, label=''):
    """drive the context through `ops`; compare at every download"""
    L = c.L
    last, same = None, False                               # the field the context must hold bit for bit, if known
    for i, (o, w) in enumerate(zip(ops, want)):
        where = '%s op %d %s' % (label, i, o['op'])
        if o.get('error'):
            with pytest.raises(L.AdiError):
                {'build': lambda: c.build(o['h'], o['q'], o['dm'], o['dv']),
                 'step': lambda: c.step(o['dt'], o['theta'], o['Tinf'], o['nsteps']),
                 'download_T': c.download, 'download_pack': lambda: c.pack(o['axis'])}[o['op']]()
        elif o['op'] == 'set_mask':
            c.set_mask(o['mask'])
        elif o['op'] == 'build':
            c.build(o['h'], o['q'], o['dm'], o['dv'])
        elif o['op'] == 'upload':
            c.upload(o['T'])
            last, same = o['T'], True
        elif o['op'] == 'step':
            c.step(o['dt'], o['theta'], o['Tinf'], o['nsteps'])
            same = same and o['nsteps'] == 0               # nsteps = 0 leaves the field bit-identical
        elif o['op'] == 'download_T':
            got = c.download()
            assert np.isfinite(w).all(), where
            e = rel_linf(got, w)
            assert e <= TOL, (where, e)
            if same:
                assert np.array_equal(got, last), where
            last, same = got, True
        else:
            co, qf = c.pack(o['axis'])
            assert np.array_equal(co, w[0]) and np.array_equal(qf, w[1]), where


def test_fuzz_programs_cover_every_rule():
    """the seeded programs together contain every input class and every state rule the fuzz is there for"""
    tags, shapes = set(), set()
    for seed in FUZZ_SEEDS:
        shape, _, ops, t = make_program(seed)
        assert 8 <= len(ops) <= 12
        tags |= t
        shapes.add(shape)
    need = {'mask:solid', 'mask:holes5', 'mask:holes30', 'mask:disk', 'dir:none', 'dir:plane_null', 'dir:rand5', 'dir:zeros',
            'err:null_field', 'err:build_before_mask', 'err:step_after_remask', 'err:download_before_upload',
            'err:pack_after_remask', 'download_pack', 'upload_after_odd_steps', 'theta:0.5', 'theta:1'}
    need |= {'gam:%g' % g for g in GAMS} | {'nsteps:%d' % k for k in range(4)}
    need |= {'%s:%s' % (a, m) for a in 'hq' for m in ('NONE', 'SCALAR', 'FIELD')}
    assert need <= tags, sorted(need - tags)
    assert shapes == set(FUZZ_SHAPES)


@pytest.mark.parametrize('seed', FUZZ_SEEDS)
def test_ctx_sequence_fuzz(seed):
    """A random program on one context (masks, per-face NONE / SCALAR / FIELD coefficients and fluxes, four kinds of Dirichlet
    data, dt on both sides of the kMixedMinTg gate, nsteps 0 ... 3, uploads between steps, refused calls), mirrored into the
    oracle: every downloaded field at rel_linf <= 1e-10, every downloaded pack bit for bit."""
    shape, dx, ops, _ = make_program(seed)
    want = run_oracle(shape, dx, ops)
    c = Ctx(shape, dx)
    try:
        run_ctx(c, ops, want, 'seed %d' % seed)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# (d): two contexts alive at once
# ---------------------------------------------------------------------------------------------------------------------
def test_two_contexts_interleaved():
    """Two contexts of different shapes -- one whose mask queues units (no promise), one all-solid (promise taken) -- stepped
    alternately, one operation of each program at a time, each against its own oracle run.  A refused call on one (its message
    lands in the shared error buffer) must not disturb the other."""
    progs = []
    for seed, (shape, mk, dk) in enumerate([((256, 16, 32), 'holes5', None), ((24, 20, 96), 'solid', 'plane')]):
        rng = np.random.default_rng(70 + seed)
        dx = 1e-3
        dm = None
        if dk:
            dm = np.zeros(shape, bool)
            dm[:, :, 0] = True
        ops = [dict(op='set_mask', mask=_mask(rng, shape, mk)),
               dict(op='build', h=[300.0, 120.0, None, 300.0, rng.uniform(50.0, 800.0, shape), 40.0],
                    q=[None, 2e4, None, None, None, None], dm=dm, dv=None, error=False),
               dict(op='upload', T=rng.uniform(20.0, 900.0, shape))]
        for gam, theta, ns in [(60.0, 0.5, 1), (GAM_TINY, 0.5, 2), (60.0, 1.0, 3), (0.3, 0.5, 2)]:
            ops.append(dict(op='step', dt=dt_of(gam, dx), theta=theta, Tinf=20.0 + seed, nsteps=ns, error=False))
            ops.append(dict(op='download_T', error=False))
        ops.insert(5, dict(op='download_pack', axis=seed, error=False))
        ops.insert(7 + seed, dict(op='step', dt=1.0, theta=0.5, Tinf=0.0, nsteps=-1, error=True))   # ADI_ERR_ARG
        progs.append((shape, dx, ops, run_oracle(shape, dx, ops)))
    ctxs = [Ctx(p[0], p[1]) for p in progs]
    try:
        for i in range(max(len(p[2]) for p in progs)):
            for n, (c, p) in enumerate(zip(ctxs, progs)):
                if i < len(p[2]):
                    run_ctx(c, p[2][i:i + 1], p[3][i:i + 1], 'ctx %d op %d' % (n, i))
                    if p[2][i].get('error'):
                        assert 'adi_ctx_step' in c.L.last_error()
    finally:
        for c in ctxs:
            c.close()
