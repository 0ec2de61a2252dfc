"""The shared cases of the bead-deposition tests (test_bead_deposit_cpu.py, test_bead_deposit_gpu.py): paths, beads, windows,
`within` and already-active cells on small grids, built from the host definition alone (no device).  Every case is checked
here, when the module is imported, for its margin: no cell centre lies within a relative 1e-9 of a boundary that decides a
birth (r2 against h2, -z against cap, z against 0), read from PathDeposit.reference_terms.  That is a condition on the inputs --
path points are off the lattice -- not a tolerance on any result."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adi_thermal_fields_amd.heat_source import ScanPath                        # noqa: E402
from adi_thermal_fields_amd.deposition import BeadProfile, PathDeposit        # noqa: E402

DX = 1e-3
TS = 1750.0
MARGIN = 1e-9
GOLDAK = dict(eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3, f_f=0.6)        # the heat source of the path: of no concern to births
SHAPES = [(24, 20, 12), (13, 11, 9), (37, 29, 45)]
PADDED_SHAPE = (70, 29, 45)
PARTITION_FACTORS = (0.11, 0.37, 1.9)                                       # dt = factor * t_end / 5


class HostGrid:
    """what PathDeposit reads of a grid without a device"""

    def __init__(self, shape, dx, mask):
        self.nx, self.ny, self.nz = shape
        self.dx, self.mask = dx, mask


def axes_of(da):
    return (1 if da == 0 else 0), (1 if da == 2 else 2)


def point(da, u, v, z):
    p = [0.0, 0.0, 0.0]
    au, av = axes_of(da)
    p[au], p[av], p[da] = u, v, z
    return tuple(p)


class Case:
    """name, grid shape, path (a ScanPath), bead, the windows [(t, dt)] to deposit in this order, `within` (bool array or None)
    and the mask that is active before the first window"""

    def __init__(self, name, shape, path, bead, windows, within, active):
        self.name, self.shape, self.path, self.bead = name, shape, path, bead
        self.windows, self.within, self.active = windows, within, active
        self.da = int(path.depth_axis)

    def whole(self):
        """one window that holds the whole path"""
        return (self.path.t_start - 0.5, (self.path.t_end - self.path.t_start) + 1.0)

    def reference(self, t, dt, active=None):
        return PathDeposit.reference(self.path, self.bead, self.shape, DX, t, dt,
                                     active=self.active if active is None else active, within=self.within)

    def margin(self):
        """the smallest relative distance of a cell centre from a deciding boundary over the case's windows and the whole path"""
        w, h = self.bead.validate()
        m = np.inf
        for t, dt in list(self.windows) + [self.whole()]:
            for _, r2, h2, z, cap in PathDeposit.reference_terms(self.path, self.bead, self.shape, DX, t, dt):
                m = min(m, float(np.abs(r2 - h2).min()) / h2, float(np.abs(-z - cap).min()) / h, float(np.abs(z).min()) / DX)
        return m


def _extents(shape, da):
    au, av = axes_of(da)
    return shape[au], shape[av], shape[da]


def _path(da, pts, speeds_powers, t_start=0.0):
    """a path through the in-plane points `pts` [(u, v)] in units of DX at depth coordinate pts' third entry (kept), leg n at
    speed and power speeds_powers[n] (power 0: a jump)"""
    z = pts[0][2]
    p = ScanPath(power=800.0, depth_axis=da, start=point(da, pts[0][0] * DX, pts[0][1] * DX, z * DX), t_start=t_start, **GOLDAK)
    for (u, v, zz), (speed, power) in zip(pts[1:], speeds_powers):
        p.line_to(point(da, u * DX, v * DX, zz * DX), speed * DX, power=power)
    return p


def _plate(shape, da, planes):
    m = np.zeros(shape, dtype=bool)
    sl = [slice(None)] * 3
    sl[da] = slice(0, planes)
    m[tuple(sl)] = True
    return m


def _half(shape, da):
    """the low half of the first in-plane axis, on every plane: part of any bead that crosses it is active already"""
    m = np.zeros(shape, dtype=bool)
    sl = [slice(None)] * 3
    sl[axes_of(da)[0]] = slice(0, shape[axes_of(da)[0]] // 2)
    m[tuple(sl)] = True
    return m


def _disk(shape, da):
    """`within`: a disk in the plane about the middle of the grid, on every plane"""
    au, av = axes_of(da)
    U, V = shape[au], shape[av]
    u = (np.arange(U) + 0.5 - 0.5 * U) / (0.43 * U)
    v = (np.arange(V) + 0.5 - 0.5 * V) / (0.43 * V)
    d = (u[:, None] ** 2 + v[None, :] ** 2) <= 1.0
    # d is indexed (u, v) with au < av: put the depth axis where it belongs
    return np.broadcast_to(np.expand_dims(d, da), shape).copy()


def build_cases():
    cases = []

    def add(name, shape, da, pts, legs, windows, profile='box', width=3.3, height=2.4, within=False, active='none', t_start=0.0):
        path = _path(da, pts, legs, t_start)
        if windows == 'whole':
            windows = [(path.t_start - 0.25, (path.t_end - path.t_start) + 0.5)]
        act = {'none': np.zeros(shape, dtype=bool), 'plate': _plate(shape, da, max(1, int(pts[0][2] - height + 0.5))),
               'half': _half(shape, da)}[active]
        cases.append(Case(name, shape, path, BeadProfile(width * DX, height * DX, profile), windows,
                          _disk(shape, da) if within else None, act))

    A = SHAPES[0]
    U, V, D = _extents(A, 2)
    top = 9.3                                              # planes 7 and 8 of 12 with a bead 2.4 cells high
    P = 800.0
    # ---- single legs: +u, -u, +v, -v, oblique; profiles, within and active cells in turn
    add('leg_plus_u', A, 2, [(3.37, 6.21, top), (17.13, 6.21, top)], [(10.0, P)], 'whole', active='plate')
    add('leg_minus_u', A, 2, [(19.41, 11.83, top), (4.27, 11.83, top)], [(10.0, P)], 'whole', profile='parabola', within=True)
    add('leg_plus_v', A, 2, [(11.79, 2.63, top), (11.79, 15.17, top)], [(10.0, P)], [(0.13, 0.41), (0.54, 0.5)], active='half')
    add('leg_minus_v', A, 2, [(12.77, 16.39, top), (12.77, 3.91, top)], [(10.0, P)], 'whole', profile='parabola', active='half')
    add('oblique', A, 2, [(4.13, 3.29, top), (18.71, 13.57, top)], [(10.0, P)], [(0.2, 0.7), (0.9, 2.0)], within=True, active='plate')
    add('oblique_parabola', A, 2, [(19.23, 4.61, top), (5.09, 15.37, top)], [(10.0, P)], 'whole', profile='parabola', width=5.1, height=3.2)
    # ---- a powered corner, a step that holds it
    corner = [(4.37, 5.21, top), (15.13, 5.21, top), (15.13, 14.63, top)]
    add('corner', A, 2, corner, [(10.0, P), (10.0, P)], [(0.8, 0.6)], active='plate')
    add('corner_parabola_within', A, 2, corner, [(10.0, P), (10.0, P)], 'whole', profile='parabola', within=True)
    # ---- two legs joined by a jump, from t = 0.25: 1.076 s, 0.3 s, 1.1 s
    jump = [(4.37, 5.21, top), (15.13, 5.21, top), (15.13, 14.21, top), (4.13, 14.21, top)]
    jl = [(10.0, P), (30.0, 0.0), (10.0, P)]
    add('jump_three_segments_one_step', A, 2, jump, jl, [(1.1, 0.8)], active='plate', t_start=0.25)
    add('jump_step_inside_the_jump', A, 2, jump, jl, [(1.35, 0.2)], t_start=0.25)
    add('jump_before_t_start', A, 2, jump, jl, [(-0.4, 0.6)], t_start=0.25)
    add('jump_after_t_end', A, 2, jump, jl, [(2.8, 0.5)], t_start=0.25)
    add('jump_whole', A, 2, jump, jl, 'whole', profile='parabola', active='half', t_start=0.25)
    # ---- the path leaves the grid through each lateral side
    add('out_u_low', A, 2, [(7.31, 8.43, top), (-4.29, 8.43, top)], [(10.0, P)], 'whole', active='plate')
    add('out_u_high', A, 2, [(15.31, 9.57, top), (U + 5.41, 9.57, top)], [(10.0, P)], 'whole', profile='parabola')
    add('out_v_low', A, 2, [(9.37, 6.29, top), (12.81, -5.23, top)], [(10.0, P)], 'whole', within=True)
    add('out_v_high', A, 2, [(13.61, 12.43, top), (10.19, V + 4.77, top)], [(10.0, P)], 'whole', active='half')
    add('oblique_leaves_the_corner', A, 2, [(15.23, 11.37, top), (U + 6.31, V + 5.19, top)], [(10.0, P)], 'whole')
    add('wholly_outside', A, 2, [(U + 5.2, 3.3, top), (U + 9.4, 9.1, top)], [(10.0, P)], 'whole')
    # ---- the depth coordinate puts part of the bead below plane 0 / above the top plane
    add('below_plane_0', A, 2, [(4.37, 7.21, 1.31), (17.13, 9.77, 1.31)], [(10.0, P)], 'whole')
    add('above_the_top', A, 2, [(4.37, 7.21, D + 1.17), (17.13, 9.77, D + 1.17)], [(10.0, P)], 'whole', profile='parabola', active='half')
    add('top_plane', A, 2, [(4.37, 7.21, D - 0.29), (17.13, 9.77, D - 0.29)], [(10.0, P)], 'whole', active='plate')
    # ---- depth axes 0 and 1: the corner and the jump in the other two planes
    for da in (0, 1):
        U1, V1, D1 = _extents(A, da)
        t1 = D1 - 2.7
        sc = lambda u, v: (2.13 + u * (U1 - 4.9), 1.87 + v * (V1 - 4.3), t1)     # noqa: E731
        add('corner_depth_axis_%d' % da, A, da, [sc(0.0, 0.1), sc(1.0, 0.1), sc(1.0, 0.9)], [(10.0, P), (10.0, P)],
            [(0.3, 0.9), (1.2, 5.0)], active='plate')
        add('jump_depth_axis_%d' % da, A, da, [sc(0.1, 0.0), sc(0.9, 0.2), sc(0.9, 0.8), sc(0.0, 1.0)], [(10.0, P), (30.0, 0.0), (10.0, P)],
            'whole', profile='parabola', within=True, active='half')
        add('out_depth_axis_%d' % da, A, da, [sc(0.5, 0.5), (U1 + 3.7, V1 + 2.9, t1)], [(10.0, P)], 'whole')
    # ---- the other shapes
    B = SHAPES[1]
    add('small_corner', B, 2, [(2.37, 2.21, 7.3), (9.13, 2.21, 7.3), (9.13, 8.63, 7.3)], [(10.0, P), (10.0, P)], 'whole',
        width=2.3, height=1.4, active='plate')
    add('small_oblique_depth_axis_0', B, 0, [(1.37, 1.21, 10.6), (8.13, 7.79, 10.6)], [(10.0, P)], 'whole', profile='parabola',
        width=3.1, height=2.3, within=True)
    C = SHAPES[2]
    add('ragged_raster', C, 2, [(5.37, 6.21, 41.3), (30.13, 6.21, 41.3), (30.13, 12.21, 41.3), (5.37, 12.21, 41.3), (2.1, 20.3, 41.3),
                                (33.9, 26.7, 41.3)],
        [(10.0, P), (30.0, 0.0), (10.0, P), (30.0, 0.0), (10.0, P)], [(0.3, 1.9), (2.2, 6.0)], width=6.2, height=3.4, active='plate')
    add('ragged_top_depth_axis_1', C, 1, [(4.37, 5.21, 29.4), (31.13, 40.77, 29.4)], [(10.0, P)], 'whole', profile='parabola',
        width=7.1, height=4.3, within=True, active='half')
    # ---- a box the library pads by itself (adi_recommended_dims: 72 x 29 x 64); 37 x 29 x 45 it leaves as it is
    add('padded_by_the_library', PADDED_SHAPE, 2, [(5.37, 6.21, 41.3), (62.13, 6.21, 41.3), (62.13, 14.21, 41.3), (8.37, 20.63, 41.3)],
        [(40.0, P), (90.0, 0.0), (40.0, P)], [(0.3, 0.9), (1.2, 3.0)], profile='parabola', width=6.2, height=3.4, within=True,
        active='plate')
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
for _c in CASES:
    assert _c.margin() >= MARGIN, (_c.name, _c.margin())
