"""Shared pieces of the MapPathSource tests (test_matmap_path_source_cpu.py, test_matmap_path_source_gpu.py): eight materials
at random under a scan path, the library's host twin of the kernel, and the windows the device tests run -- each named for the
property of the launch it was built for, which `stage_cases` states and the GPU test asserts from `window()` before it launches."""
import ctypes
import zlib

import numpy as np

import matmap_eight_cases as ec
import scan_cases as sc
import scan_source_cases as ssc
from scan_cases import DT, DX

MATERIALS8 = ec.MATERIALS8
C8 = np.array([rho * cp for rho, cp, _ in MATERIALS8])
WIDE_SHAPE = (12, 14, 150)                                  # a leg along axis 2: the one box wider than a wave there


def ids_and_field(shape, mask, seed=0):
    """(ids, R0): ids uniform on 0 .. 7 with 255 off the mask, a field uniform on [20, 1500]"""
    rng = np.random.default_rng(zlib.crc32(repr(('path', tuple(shape), seed)).encode()))
    ids = rng.integers(0, 8, shape).astype(np.uint8)
    ids[~np.asarray(mask, dtype=bool)] = 255
    return ids, rng.uniform(20.0, 1500.0, shape)


def bare_map(grid, materials=MATERIALS8):
    """a MaterialMap without a device: the attributes the checks and `window` read"""
    from adi_thermal_fields_amd.packs import MaterialMap, Material
    mm = MaterialMap.__new__(MaterialMap)
    mm.grid, mm.materials = grid, tuple(Material(*m) for m in materials)
    mm.mat, mm.packs = mm.materials[0], (object(), object(), object())
    return mm


def host_twin(src, g, ids, R0, t, dt, C=C8):
    """(R0 after adi_matmap_scan_add_r0_host, the box as ((i0, i1), (j0, j1), (k0, k1))); R0 itself is not written"""
    from adi_thermal_fields_amd._lib import lib, check
    out = np.array(R0, dtype=np.float64, order='C')
    mask = np.ascontiguousarray(np.asarray(g.mask, dtype=bool), dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    box = (ctypes.c_int * 6)()
    Cv = (ctypes.c_double * len(C))(*C)
    check(lib.adi_matmap_scan_add_r0_host(*src._path_args(src._h_table.ctypes.data), out.ctypes.data, mask.ctypes.data,
                                          ids.ctypes.data, int(g.nx), int(g.ny), int(g.nz), float(g.dx), float(t), float(dt),
                                          len(C), Cv, box))
    return out, ((box[0], box[1]), (box[2], box[3]), (box[4], box[5]))


def _axis0_edges(hip, shape):
    """legs along +v hard against the low and the high face of axis 0"""
    nx, ny, nz = shape
    leg = lambda x: sc.leg_path(hip, sc.SHAPE, (x, 0.3 * ny * DX, 0.5 * nz * DX), 90.0, 8 * DX, 8 * DX / (0.8 * DT), t_start=0.1 * DT)
    return {'axis0_low': leg(1.5 * DX), 'axis0_high': leg((nx - 1.5) * DX)}


def _wide(hip):
    """depth along axis 0, a leg of 110 cells along axis 2 (the second in-plane axis) in one step"""
    nx, ny, nz = WIDE_SHAPE
    p = hip.ScanPath(power=800.0, depth_axis=0, start=((nx - 2) * DX, 0.5 * ny * DX, 20 * DX), t_start=0.0, **sc.SMALL)
    return p.line_to(((nx - 2) * DX, 0.5 * ny * DX, 130 * DX), 110 * DX / DT)


def stage_cases(hip):
    """[(name, path, shape, t, dt, want)]: `want` maps a property of the window to the value the test asserts --
    segs: powered pieces in the step; clip: (axis, 'lo' / 'hi') faces of the grid the box touches; thin / wide: the box's extent
    along axis 2 is below / above 64; depth: the path's depth axis"""
    from test_scan_path_gpu import _edge_paths, _two_leg_path, _window_path
    C, E, A = ssc.CORNER_SHAPE, ssc.EDGE_SHAPE, ssc.AXIS_SHAPE
    wp = _window_path(hip, C)
    two = _two_leg_path(hip, C, sc.SHAPE, 0.25 * DT)
    out = [('inside_one_leg', wp, C, 3.0 * DT, DT, dict(segs=1, thin=True)),
           ('corner_three_segments', wp, C, 4.6 * DT, DT, dict(segs=2, range3=True)),
           ('corner_two_legs', two, C, 0.6 * DT, DT, dict(segs=2)),
           ('whole_path', wp, C, wp.t_start - 0.5 * DT, (wp.t_end - wp.t_start) + DT, dict(segs=3, whole=True))]
    ed = dict(_edge_paths(hip, E), **_axis0_edges(hip, E))
    clips = {'axis0_low': [(0, 'lo')], 'axis0_high': [(0, 'hi')], 'axis1_low': [(1, 'lo')], 'axis1_high': [(1, 'hi')],
             'axis2_low': [(2, 'lo')], 'axis2_high': [(2, 'hi')], 'both_sides': [(1, 'lo'), (1, 'hi'), (2, 'lo'), (2, 'hi')]}
    out += [('edge_' + n, ed[n], E, 0.0, DT, dict(segs=1, clip=c)) for n, c in clips.items()]
    out += [('depth_axis_%d' % da, ssc.oblique(hip, da), A, 0.0, DT, dict(segs=1, depth=da)) for da in (0, 1, 2)]
    out.append(('dwell_with_power', ssc.dwell(hip), A, 0.2 * DT, DT, dict(segs=2, dwell=True)))
    out.append(('wide_along_axis_2', _wide(hip), WIDE_SHAPE, 0.0, DT, dict(segs=1, wide=True)))
    return out


STAGE_IDS = (['inside_one_leg', 'corner_three_segments', 'corner_two_legs', 'whole_path'] +
             ['edge_' + n for n in ('axis0_low', 'axis0_high', 'axis1_low', 'axis1_high', 'axis2_low', 'axis2_high', 'both_sides')] +
             ['depth_axis_%d' % d for d in (0, 1, 2)] + ['dwell_with_power', 'wide_along_axis_2'])


def check_window(path, shape, t, dt, want, window):
    """the case is what its name says: asserted from the path's own pieces and the library's window"""
    k0, k1, box = window
    pieces = [k for k in range(path.n_segments) if path._piece(k, t, t + dt) is not None]
    assert len(pieces) == want['segs'], (pieces, want)
    assert all(lo < hi for lo, hi in box)
    if want.get('range3'):
        assert k1 - k0 >= 3                                 # the jump between the two legs is in the range
    if want.get('whole'):
        assert (k0, k1) == (0, path.n_segments) and t < path.t_start and t + dt > path.t_end
    for axis, side in want.get('clip', ()):
        assert (box[axis][0] == 0) if side == 'lo' else (box[axis][1] == shape[axis]), (axis, side, box)
    if want.get('thin'):
        assert box[2][1] - box[2][0] < 64
    if want.get('wide'):
        assert box[2][1] - box[2][0] > 64
    if 'depth' in want:
        assert path.depth_axis == want['depth']
    if want.get('dwell'):
        assert 0.0 in ssc.deltas(path, t, dt)
