"""GPU: the sequence of engine and comm calls every rank of a SlabStepper makes with the HIP engine is the recorded one
(slab_trace.py; slab_trace_gpu.json): the branches the reference engine of test_slab_trace_cpu.py lacks -- the all-solid hint
(box_hint), padded planes (plane_dims), the dot-product pass A with its plane chunks (dots_ichunk), the fused and dots support
predicates, and the heat source on both routes (source_lines0 after the zero-boundary solve, source_add_r0 into R0).  Ranks in
one process over LocalComm, three steps per case; the grids are the small ones of test_dist_slab_gpu.py and
test_slab_source_gpu.py.  (A recorded comm is no TorchDistComm, so the exchanges run on the main stream here; the stream path is
test_dist_slab_gpu.test_slab_step_over_real_rccl_self_loop's.)"""
import os

import numpy as np
import pytest

import slab_trace

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAT = dict(rho=7800.0, cp=490.0, k=54.0)
ALPHA = 54.0 / (7800.0 * 490.0)


def _grid(shape, kind, cfl, seed, dx=1e-3):
    rng = np.random.default_rng(seed)
    mask = np.ones(shape, bool)
    neumann, robin = {'x-': 4e5}, 350.0
    if kind == 'holes':
        mask = rng.random(shape) > 0.05
    elif kind == 'ellipsoid':
        g = np.meshgrid(*[(np.arange(s) + 0.5) / s - 0.5 for s in shape], indexing='ij')
        mask = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 0.23
    else:
        neumann, robin = {'x-': 3e5, 'x+': 1e5, 'y+': 2e5}, rng.uniform(100.0, 600.0, shape)
    return dict(shape=shape, dx=dx, mask=mask, dir_mask=None, dir_value=None, neumann=neumann, robin_h=robin, Tinf=20.0,
                theta=0.5, dt=cfl * dx * dx / ALPHA, T0=rng.uniform(20.0, 1200.0, shape))


def _source_case(shape, cfl, kind, seed, x0, origin=None):
    """a grid of test_slab_source_gpu.py with a source that travels 8 cells along the sharded axis within 4 steps from plane x0"""
    import test_slab_source_gpu as ssg
    c = dict(ssg._case(shape, cfl, kind, seed=seed), dx=ssg.DX)
    kw = {} if origin is None else dict(origin=tuple(o * ssg.DX for o in origin))
    c['source'] = ssg._source(c, x0 * ssg.DX, vx=8.0 * ssg.DX / (4 * c['dt']), **kw)
    return c


HOLES, SOLID = ((256, 10, 40), 'holes'), ((256, 16, 64), 'solid')
SRC_SOLID, SRC_HOLES = ((128, 16, 32), 3.0, 'robin_field', 1, 58.0), ((256, 10, 40), 'holes', 4, 60.0, (60.0, 5.0, 30.0))

# name -> (() -> case dict, slab sizes, options, expected axis0_mode)
CASES = {
    'window': (lambda: _grid(*HOLES, 0.1, 7), [64] * 4, {}, 'window'),
    'slab': (lambda: _grid(*HOLES, 3.0, 7), [64] * 4, {}, 'slab'),
    'slab_no_dots': (lambda: _grid(*HOLES, 3.0, 7), [64] * 4, dict(allow_dots=False), 'slab'),
    'slab_recompute_r0': (lambda: _grid(*HOLES, 3.0, 7), [64] * 4, dict(allow_dots=False, keep_r0=False), 'slab'),
    'slab_separate': (lambda: _grid(*HOLES, 3.0, 7), [64] * 4, dict(allow_dots=False, allow_fused=False), 'slab'),
    'exact': (lambda: _grid(*HOLES, 300.0, 7), [64] * 4, {}, 'exact'),
    'exact_no_dots': (lambda: _grid(*HOLES, 300.0, 7), [64] * 4, dict(allow_dots=False), 'exact'),
    # all-solid slabs kept off the deferred form: the dot-product pass A, explicit stage in chunks of planes around the halo wait
    'dots_slab': (lambda: _grid((128, 16, 32), 'solid', 3.0, 5), [64, 64], dict(allow_deferred=False), 'slab'),
    'dots_exact_128_planes': (lambda: _grid((384, 8, 32), 'solid', 150.0, 9), [128] * 3, dict(allow_deferred=False), 'exact'),
    'deferred': (lambda: _grid(*SOLID, 3.0, 31), [64] * 4, {}, 'deferred'),
    'deferred_unfused': (lambda: _grid(*SOLID, 3.0, 31), [64] * 4, dict(allow_fused=False), 'deferred'),
    'deferred_padded': (lambda: _grid((192, 24, 40), 'solid', 1.0, 31), [64] * 3, {}, 'deferred'),
    'deferred_exact': (lambda: _grid(*SOLID, 300.0, 31), [64] * 4, {}, 'deferred_exact'),
    'deferred_lines': (lambda: _grid((256, 16, 64), 'holes', 0.3, 336), [64] * 4, dict(allow_deferred_lines=True), 'deferred_lines'),
    'slab_padded_unfused': (lambda: _grid((128, 100, 37), 'ellipsoid', 3.0, 267), [64, 64], dict(allow_fused=False), 'slab'),
    'source_deferred': (lambda: _source_case(*SRC_SOLID), [64, 64], {}, 'deferred'),
    'source_deferred_unfused': (lambda: _source_case(*SRC_SOLID), [64, 64], dict(allow_fused=False), 'deferred'),
    'source_deferred_exact': (lambda: _source_case((64, 16, 32), 200.0, 'robin_field', 2, 30.0), [16] * 4, {}, 'deferred_exact'),
    'source_window': (lambda: _source_case((256, 10, 40), 0.1, *SRC_HOLES[1:]), [64] * 4, dict(allow_deferred=False), 'window'),
    'source_slab': (lambda: _source_case((256, 10, 40), 3.0, *SRC_HOLES[1:]), [64] * 4, dict(allow_deferred=False), 'slab'),
    'source_exact': (lambda: _source_case((256, 10, 40), 300.0, *SRC_HOLES[1:]), [64] * 4, dict(allow_deferred=False), 'exact'),
    # (a birth loop re-sets the mask between steps: the second and third plan are quick ones)
    'source_slab_quick_replan': (lambda: _source_case((256, 10, 40), 3.0, *SRC_HOLES[1:]), [64] * 4,
                                 dict(allow_deferred=False, set_mask_between=True), 'slab'),
}


def run_case(name):
    """-> (the whole final field, [(axis0_mode, fused, dots, quick) of every rank's last plan], the ranks' logs)"""
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import dist_slab
    make, sizes, opts, _ = CASES[name]
    c = make()
    src = c.get('source')

    def fn(rank, comm, wrap):
        i0 = sum(sizes[:rank]); i1 = i0 + sizes[rank]

        def loc(a):
            return a if (a is None or np.isscalar(a)) else np.asarray(a)[i0:i1]
        neumann = None if c['neumann'] is None else {f: loc(v) for f, v in c['neumann'].items()}
        robin = {f: loc(v) for f, v in c['robin_h'].items()} if isinstance(c['robin_h'], dict) else loc(c['robin_h'])
        st = dist_slab.SlabStepper(c['mask'][i0:i1], c['dx'], hip.Material(**MAT), hip.Params(c['dt'], c['theta']), c['Tinf'],
                                   dir_mask=loc(c['dir_mask']), dir_value=loc(c['dir_value']), neumann=neumann, robin_h=robin,
                                   comm=comm, engine=wrap(dist_slab.HipEngine()), source=src)
        st._allow_fused = bool(opts.get('allow_fused', True))
        st._allow_dots = bool(opts.get('allow_dots', True))
        st._keep_r0 = bool(opts.get('keep_r0', True))
        st._allow_deferred = bool(opts.get('allow_deferred', True))
        st._allow_deferred_lines = bool(opts.get('allow_deferred_lines', False))
        st._deferred_lines_cost_ratio = float('inf')
        T = hip.to_device(np.ascontiguousarray(c['T0'][i0:i1]))
        for s in range(3):
            if opts.get('set_mask_between') and s > 0:
                st.set_mask(c['mask'][i0:i1])
            T = st.step(T, prefetch_halo=s < 2, t=None if src is None else s * c['dt'])
        p = st._a0
        return T.get(), (st.axis0_mode, bool(p['fused']), bool(p['dots']), bool(p.get('quick')))
    res, logs = slab_trace.trace_ranks(len(sizes), fn)
    return np.concatenate([r[0] for r in res], axis=0), [r[1] for r in res], logs


@pytest.fixture(scope='module')
def recorded():
    return slab_trace.load(os.path.join(HERE, 'slab_trace_gpu.json'))


@pytest.mark.parametrize('name', list(CASES))
def test_every_rank_makes_the_recorded_calls(recorded, name):
    _, plans, logs = run_case(name)
    opts, mode = CASES[name][2:4]
    assert {p[0] for p in plans} == {mode}, plans
    assert len(set(plans)) == 1, plans                               # ... and on how pass A runs
    _, fused, dots, quick = plans[0]
    if name.startswith('dots'):
        assert dots and not fused, plans
    if name.startswith('source') or 'allow_dots' in opts:
        assert not dots, plans
    if name.startswith('source') and not mode.startswith('deferred') or 'allow_fused' in opts:
        assert not fused, plans                                     # with a source the two-pass forms read R0 as stored
    assert quick == bool(opts.get('set_mask_between')), plans
    slab_trace.assert_same(logs, recorded[name], name)
