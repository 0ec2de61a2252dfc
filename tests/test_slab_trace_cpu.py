"""CPU: the sequence of engine and comm calls every rank of a SlabStepper makes, in each axis-0 form, is the recorded one
(slab_trace.py; slab_trace_cpu.json).  Reference engine, ranks in one process over LocalComm, three steps per case so that
plan reuse, the g-only exchange after the first one (matrix_sent) and the halo prefetch all show.  The cases are the smallest
of test_dist_slab_cpu.py that select each form."""
import os
import sys

import numpy as np
import pytest
import torch

import slab_trace
from test_dist_slab_cpu import _case

HERE = os.path.dirname(os.path.abspath(__file__))
DT_SEQ = [1.0, 1.0, 0.02, 0.5, 30.0, 0.02, 3000.0, 2.0, 0.01]      # test_short_lived_plans_are_made_without_measuring

# name -> (case, slab sizes, options as in test_dist_slab_cpu._worker, expected axis0_mode)
CASES = {
    'window': ('decay:128', [64, 64], {}, 'window'),
    'window_unfused': ('decay:128', [64, 64], dict(allow_fused=False), 'window'),
    'slab': ('decay:72', [24] * 3, {}, 'slab'),
    'slab_no_dots': ('decay:72', [24] * 3, dict(allow_dots=False), 'slab'),
    'slab_recompute_r0': ('decay:72', [24] * 3, dict(keep_r0=False, allow_dots=False), 'slab'),
    'slab_unfused': ('decay:72', [24] * 3, dict(allow_fused=False), 'slab'),
    'exact': ('stiff:64', [16] * 4, {}, 'exact'),
    'deferred': ('solid:128:0.1', [64, 64], {}, 'deferred'),
    'deferred_unfused': ('solid:128:0.1', [64, 64], dict(allow_fused=False), 'deferred'),
    'deferred_exact': ('solid:24:50', [12, 12], {}, 'deferred_exact'),
    'slab_uneven': ('decay:126', [64, 62], {}, 'slab'),
    'deferred_lines': ('decay:128', [64, 64], dict(allow_deferred_lines=True), 'deferred_lines'),
    'deferred_lines_cost_rule': ('cavity:128:0.5', [64, 64], dict(allow_deferred_lines=True, cost_rule=True), 'deferred_lines'),
    # (every line of this solid is flagged; the middle rank carries both sides' flagged lines, 24 B x 2 x 20 lines x K rows against
    # 17 B x 20 lines x 2 K rows of pass A: the cost rule declines there, and with it, behind the form's all-gather, everywhere)
    'deferred_lines_declined_by_cost_rule': ('decay:192', [64] * 3, dict(allow_deferred_lines=True, cost_rule=True), 'window'),
    'quick_replan': ('decay:64', [32, 32], dict(dt_seq=DT_SEQ), None),
    'no_quick_replan': ('decay:64', [32, 32], dict(dt_seq=DT_SEQ, quick_replan=False), None),
    'padded': ('decay:128', [64, 64], dict(pad=(2, 3)), 'window'),
}


def run_case(name):
    """-> (the whole final field, per step the (axis0_mode, quick) every rank reported, the ranks' logs)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from adi_thermal_fields_amd import dist_slab
    from cpu_engine import CpuEngine
    from oracle import adi_oracle as orc
    case_name, sizes, opts, _ = CASES[name]
    c = _case(case_name)
    seq = opts.get('dt_seq')
    nsteps = len(seq) if seq else 3

    def fn(rank, comm, wrap):
        i0 = sum(sizes[:rank]); i1 = i0 + sizes[rank]

        def loc(a):
            return a if (a is None or np.isscalar(a)) else np.asarray(a)[i0:i1]
        neumann = None if c['neumann'] is None else {f: loc(v) for f, v in c['neumann'].items()}
        engine = CpuEngine()
        if opts.get('pad'):
            dy, dz = opts['pad']
            engine.plane_dims = lambda ny, nz: (ny + dy, nz + dz)
        st = dist_slab.SlabStepper(c['mask'][i0:i1], c['dx'], orc.Material(**c['mat']), orc.Params(c['dt'], c['theta']), c['Tinf'],
                                   dir_mask=loc(c['dir_mask']), dir_value=loc(c['dir_value']), neumann=neumann,
                                   robin_h=loc(c['robin_h']), comm=comm, engine=wrap(engine))
        assert st._padded == bool(opts.get('pad'))
        st._allow_fused = bool(opts.get('allow_fused', True))
        st._keep_r0 = bool(opts.get('keep_r0', True))
        st._allow_dots = bool(opts.get('allow_dots', True))
        st._allow_deferred_lines = bool(opts.get('allow_deferred_lines', False))
        st._deferred_lines_cost_ratio = 1.0 if opts.get('cost_rule') else float('inf')
        st._allow_quick_replan = bool(opts.get('quick_replan', True))
        T = torch.from_numpy(np.ascontiguousarray(c['T0'][i0:i1]))
        modes = []
        for s in range(nsteps):
            if seq:
                st.params.dt = c['dt'] * seq[s]
            T = st.step(T, prefetch_halo=s + 1 < nsteps and not seq)
            modes.append((st.axis0_mode, bool(st._a0.get('quick'))))
        return T.numpy().copy(), modes
    res, logs = slab_trace.trace_ranks(len(sizes), fn)
    assert all(r[1] == res[0][1] for r in res), [r[1] for r in res]          # the ranks agree on the form of every step
    return np.concatenate([r[0] for r in res], axis=0), res[0][1], logs


@pytest.fixture(scope='module')
def recorded():
    return slab_trace.load(os.path.join(HERE, 'slab_trace_cpu.json'))


@pytest.mark.parametrize('name', list(CASES))
def test_every_rank_makes_the_recorded_calls(recorded, name):
    _, modes, logs = run_case(name)
    want = CASES[name][3]
    if want is not None:
        assert modes == [(want, False)] * 3, modes
    else:
        # an event loop: the first plan is measured, the later ones are quick (unless switched off), the sequence of time
        # steps walks through the forms (measured, two ranks never need 'exact': no slab has neighbours on both sides)
        quick = CASES[name][2].get('quick_replan', True)
        assert not modes[0][1] and all(q == quick for _, q in modes[2:]), modes
        assert ({'exact', 'window'} if quick else {'slab', 'window'}) <= {m for m, _ in modes}, modes
    slab_trace.assert_same(logs, recorded[name], name)
