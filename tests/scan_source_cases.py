"""Shared cases of the ScanPathSource tests (test_scan_source_cpu.py, test_scan_source_gpu.py): a path, a grid shape, a window
and the bar its device (or library) evaluation is held to against the host definition ScanPath.sample_step.

The bars: the evaluators differ from the host definition by the rounding of erf and exp only, and the error of an erf difference
grows as 1/delta, delta = travel of a piece over min(c_f, c_r).  With the host erf perturbed by +-16 ulp (OpenCL's accuracy bound
for erf) the relative L-inf of the field is 2.5e-15 at delta = 2.4, 3.4e-14 at 0.1, 3.6e-13 at 1e-2 and 1.7e-12 at 2e-3.  So a
case whose every powered piece has delta >= 0.1, or takes no erf at all (a dwell, Simpson's rule below delta = 1e-3), is held to
BAR = 1e-12, the project's one-step bar; a case with a piece in [1e-3, 0.1) to BAR_SMALL_DELTA = 1e-10."""
import numpy as np

import scan_cases as sc
from scan_cases import DT, DX
from test_scan_path_gpu import EDGES, WINDOWS, _edge_paths, _two_leg_path, _window_path

BAR = 1e-12
BAR_SMALL_DELTA = 1e-10

CORNER_SHAPE = (37, 29, 45)
EDGE_SHAPE = (33, 21, 19)
AXIS_SHAPE = (30, 28, 26)
BRANCH_SHAPE = (24, 20, 18)


def case_mask(shape):
    """the mask of the Goldak tests: random holes, two planes off on top, a hole under the path"""
    return sc.make_case(shape)[0]


def window_time(path, when):
    t = {'tab1': path.table()[1, 0], 'end': path.t_end + 0.25 * DT}.get(when, None)
    return when * DT if t is None else t


def oblique(hip, depth_axis):
    """a leg at 30 degrees in the plane normal to depth_axis, just under the high face along it, delta about 2.7 per step"""
    n = AXIS_SHAPE
    au, av = sc.axes_of(depth_axis)
    lo = (0.3 * n[au] * DX, 0.3 * n[av] * DX, (n[depth_axis] - 2) * DX)
    return sc.leg_path(hip, sc.SHAPE, lo, 30.0, 8 * DX, 8 * DX / (0.8 * DT), depth_axis=depth_axis, t_start=0.1 * DT)


def dwell(hip):
    """a leg, then a dwell with power that keeps the leg's direction: the window below holds the end of the leg and the dwell"""
    n = BRANCH_SHAPE
    p = sc.leg_path(hip, sc.SHAPE, (0.4 * n[0] * DX, 0.4 * n[1] * DX, (n[2] - 2) * DX), 20.0, 4 * DX, 4 * DX / (0.7 * DT))
    return p.dwell(2.0 * DT, power=500.0)


def slow_leg(hip, delta):
    """one leg whose pieces of a whole step travel delta * min(c_f, c_r)"""
    n = BRANCH_SHAPE
    cmin = min(sc.SHAPE['c_f'], sc.SHAPE['c_r'])
    v = delta * cmin / DT
    return sc.leg_path(hip, sc.SHAPE, (0.5 * n[0] * DX, 0.4 * n[1] * DX, (n[2] - 2) * DX), 15.0, 3.0 * v * DT, v)


def bar_of(path, t, dt):
    """the rule above, from the step's own pieces"""
    return BAR_SMALL_DELTA if any(1e-3 <= d < 0.1 for d in deltas(path, t, dt)) else BAR


def cases(hip):
    """[(name, path, shape, mask or None, t, dt, bar, deposits)]"""
    out = [('corner', _two_leg_path(hip, CORNER_SHAPE, sc.SHAPE, 0.25 * DT), CORNER_SHAPE, None, 0.6 * DT),
           ('corner_masked', _two_leg_path(hip, CORNER_SHAPE, sc.SHAPE, 0.25 * DT), CORNER_SHAPE, case_mask(CORNER_SHAPE), 0.6 * DT)]
    for name, when, segs in WINDOWS:
        p = _window_path(hip, CORNER_SHAPE)
        out.append(('window_' + name, p, CORNER_SHAPE, None, window_time(p, when)))
    for da in (0, 1, 2):
        out.append(('depth_axis_%d' % da, oblique(hip, da), AXIS_SHAPE, None, 0.0))
    out.append(('dwell_with_power', dwell(hip), BRANCH_SHAPE, None, 0.2 * DT))
    out.append(('simpson_delta_5e-4', slow_leg(hip, 5e-4), BRANCH_SHAPE, None, 0.5 * DT))
    out.append(('erf_delta_2e-3', slow_leg(hip, 2e-3), BRANCH_SHAPE, None, 0.5 * DT))
    for name in EDGES:
        out.append(('edge_' + name, _edge_paths(hip, EDGE_SHAPE)[name], EDGE_SHAPE, None, 0.0))
    return [c + (DT, bar_of(c[1], c[4], DT), bool(deltas(c[1], c[4], DT))) for c in out]


CASE_IDS = (['corner', 'corner_masked'] + ['window_' + w[0] for w in WINDOWS] + ['depth_axis_%d' % d for d in (0, 1, 2)] +
            ['dwell_with_power', 'simpson_delta_5e-4', 'erf_delta_2e-3'] + ['edge_' + e for e in EDGES])


def support_boxes(path, shape, t, dt):
    """bool array: the cells inside the _index_box of some piece of the step [t, t + dt]"""
    inside = np.zeros(shape, dtype=bool)
    for k in range(path.n_segments):
        pc = path._piece(k, t, t + dt)
        if pc is not None:
            inside[path._index_box(k, pc, shape, DX)] = True
    return inside


def deltas(path, t, dt):
    """travel over min(c_f, c_r) of every powered piece of the step"""
    cmin = min(path.c_f, path.c_r)
    return [path._seg[k][4] * pc[2] / cmin for k in range(path.n_segments) for pc in [path._piece(k, t, t + dt)] if pc is not None]
