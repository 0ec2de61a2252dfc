"""Recorder for the slab decomposition's call sequence (tests only): wraps the engine and the comm of every rank and logs, per
rank and in order, each call they receive -- method name, scalar arguments, shapes of tensor arguments, None-ness of optional
ones, scalar results -- and no pointers; `vec`, the allocation of a zeroed plan-time buffer, is the one call left out (it neither
launches a step's kernel nor exchanges anything, and how many flag buffers a planner keeps is its own business).  The ranks of
a step must issue the same exchanges with the same sizes in the same order; a refactoring of SlabStepper must not move a launch.  The expected logs (slab_trace_cpu.json, slab_trace_gpu.json) were
recorded with this file on the commit before SlabStepper was split up:

    python tests/slab_trace.py cpu|gpu          rewrites the file from the tree it runs in
"""
import json
import os
import threading

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _describe(v):
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, (np.bool_, np.integer)):
        return v.item()
    if isinstance(v, (float, np.floating)):
        return float('%.12g' % float(v))            # (a device- or LAPACK-computed scalar may differ in its last bits across hosts)
    if isinstance(v, torch.Tensor):
        return 'T%s:%s' % (list(v.shape), str(v.dtype).split('.')[-1])
    if isinstance(v, np.ndarray):
        return 'A%s:%s' % (list(v.shape), v.dtype)
    if isinstance(v, (tuple, list)):
        return [_describe(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _describe(x) for k, x in v.items()}
    if all(hasattr(v, a) for a in ('nx', 'ny', 'nz', 'sx')):
        return 'L(%d,%d,%d;%d)' % (v.nx, v.ny, v.nz, v.sx)
    return '<%s>' % type(v).__name__


class Recorder:
    """stands in for an engine or a comm: attributes read and written through, public method calls logged to `log`"""

    def __init__(self, obj, log, tag):
        object.__setattr__(self, '_obj', obj)
        object.__setattr__(self, '_log', log)
        object.__setattr__(self, '_tag', tag)

    def __setattr__(self, name, value):
        setattr(self._obj, name, value)

    def __getattr__(self, name):
        v = getattr(self._obj, name)                 # (AttributeError passes: SlabStepper asks engines what they can do with hasattr)
        if name.startswith('_') or name == 'vec' or not callable(v) or isinstance(v, type):
            return v

        def call(*args, **kw):
            entry = [self._tag + '.' + name, [_describe(a) for a in args], {k: _describe(a) for k, a in sorted(kw.items())}]
            self._log.append(entry)
            res = v(*args, **kw)
            if isinstance(res, (bool, int, float, tuple, np.bool_, np.integer, np.floating)):
                entry.append(_describe(res))
            return res
        return call


def trace_ranks(world, fn, timeout=300):
    """fn(rank, comm, wrap) on `world` threads, one per rank, over dist_slab.LocalComm; `comm` records, and so does
    wrap(engine) -> ([fn's results], [each rank's log as a list of JSON strings])"""
    from adi_thermal_fields_amd import dist_slab
    comms = dist_slab.LocalComm.make(world)
    logs = [[] for _ in range(world)]
    out, errs = [None] * world, []

    def work(rank):
        try:
            if torch.cuda.is_available():
                torch.cuda.set_device(0)
            out[rank] = fn(rank, Recorder(comms[rank], logs[rank], 'comm'), lambda e: Recorder(e, logs[rank], 'engine'))
        except Exception as e:   # surface the failure and release the other ranks
            errs.append(e)
            comms[rank].sh.barrier.abort()
    ths = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=timeout)
    if errs:
        raise errs[0]
    return out, [[json.dumps(e, sort_keys=True) for e in log] for log in logs]


# the file: {"calls": [every distinct call, as a string], "cases": {case: [per rank: indices into calls]}}
def save(path, traces):
    calls, index = [], {}
    cases = {}
    for name, logs in traces.items():
        cases[name] = [[index.setdefault(s, len(index)) for s in log] for log in logs]
    calls = sorted(index, key=index.get)
    with open(path, 'w') as f:
        json.dump(dict(calls=calls, cases=cases), f, separators=(',', ':'))
        f.write('\n')


def load(path):
    with open(path) as f:
        d = json.load(f)
    return {name: [[d['calls'][i] for i in log] for log in logs] for name, logs in d['cases'].items()}


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for rank, (g, w) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, '%s, rank %d, call %d:\n  now      %s\n  recorded %s' % (what, rank, i, a, b)
        assert len(g) == len(w), '%s, rank %d: %d calls now, %d recorded; first extra: %s' % (
            what, rank, len(g), len(w), (g[len(w):] or w[len(g):])[0])


if __name__ == '__main__':
    import sys
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
    kind = sys.argv[1]
    mod = __import__('test_slab_trace_' + kind)
    save(os.path.join(HERE, 'slab_trace_%s.json' % kind), {name: mod.run_case(name)[2] for name in mod.CASES})
