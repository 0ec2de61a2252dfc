"""GPU: the solid voxeliser (adi_thermal_fields_amd.voxelize, csrc/adi_voxelize.hip) against the CPU statement of its
definition (tests/voxelize_ref.py, pinned by test_voxelize_cpu.py), bit for bit with no cell left out, and against
closed-form inside tests that do not go through that statement.

Bounds.  Device against CPU statement: equality of every cell and of the leak counts; both do the same IEEE operations
in the same order, and nothing is summed, so there is no rounding to allow for.  Against a closed form a cell may be left
out when its centre lies within 1e-9 dx of the surface (there the rounded depth decides); at most 1e-4 of the grid's cells
may be, and the tests assert that share.  For the tilted prism as given no cell is that near.
"""
import os

import numpy as np
import pytest

import cases
import voxelize_ref as vr
from helpers import rel_linf
from stlcorr_meshes import _fuzz_mask, box_triangles, plate_triangles, tube_triangles

pytestmark = pytest.mark.gpu

AXES = [0, 1, 2, 'majority']


def _device(tri, org, dx, shape, axis):
    from adi_thermal_fields_amd.voxelize import voxelize_solid
    got, leaks = voxelize_solid(vr_mesh(tri), org, dx, shape, axis=axis, return_leaks=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and got.shape == tuple(shape)
    return got, leaks


def vr_mesh(tri):
    return type('Mesh', (), {'triangles': np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)})()


_CPU = {}


def _cpu(tri, org, dx, shape, axis):
    """the CPU statement, each (mesh, grid, axis) worked out once: 'majority' reuses the three axes"""
    if axis == 'majority':
        res = [_cpu(tri, org, dx, shape, a) for a in range(3)]
        return sum(m.astype(np.int8) for m, _ in res) >= 2, tuple(l for _, l in res)
    key = (hash(np.ascontiguousarray(tri).tobytes()), tuple(float(v) for v in org), float(dx), tuple(shape), axis)
    if key not in _CPU:
        _CPU[key] = vr.voxelize(tri, org, dx, shape, axis)
    return _CPU[key]


def _same(tri, org, dx, shape, axis, what=''):
    got, leaks = _device(tri, org, dx, shape, axis)
    want, want_leaks = _cpu(tri, org, dx, shape, axis)
    bad = int((got != want).sum())
    print('VOXELIZE %s axis %s shape %s: %d triangles, %d solid, %d cells differ, leaks %s (CPU %s)'
          % (what, axis, tuple(shape), len(tri), int(want.sum()), bad, leaks, want_leaks))
    assert bad == 0, (what, axis, bad)
    assert leaks == want_leaks, (what, axis, leaks, want_leaks)
    return got, leaks


@pytest.mark.parametrize('axis', AXES)
@pytest.mark.parametrize('case', vr.dyadic_cases(), ids=lambda c: c[0])
def test_dyadic_cases_equal_the_cpu_statement(case, axis):
    name, tri, org, dx, shape = case
    got, leaks = _same(tri, org, dx, shape, axis, name)
    assert got.any() and not np.any(leaks)


@pytest.mark.parametrize('axis', AXES)
@pytest.mark.parametrize('kind', ['holes', 'walls'])
def test_mask_to_surface_to_mask(kind, axis):
    shape, dx = (37, 29, 50), 1e-3
    rng = np.random.default_rng(5)
    mask = _fuzz_mask(kind, shape, rng)
    org = np.array([0.0123, -0.004, 0.0007])
    tri = plate_triangles(mask, [org[a] + np.arange(shape[a] + 1) * dx for a in range(3)])
    got, leaks = _device(tri, org, dx, shape, axis)
    assert np.array_equal(got, mask) and not np.any(leaks)
    # centres shifted by -dx/2 onto the mesh planes: compared with the CPU statement, and where the shifted centre formula
    # lands exactly on the planes (the lattice origin) with the mask moved by one voxel
    big = tuple(s + 1 for s in shape)
    _same(tri, org - dx / 2, dx, big, axis, kind + ' on planes')
    dx2 = 2.0 ** -10
    org2 = np.array([3, -2, 5]) * dx2
    tri2 = plate_triangles(mask, [org2[a] + np.arange(shape[a] + 1) * dx2 for a in range(3)])
    got, leaks = _device(tri2, org2 - dx2 / 2, dx2, big, axis)
    assert np.array_equal(got[:-1, :-1, :-1], mask) and not np.any(leaks)
    assert not got[-1].any() and not got[:, -1].any() and not got[:, :, -1].any()


@pytest.mark.parametrize('axis', AXES)
def test_cut_box_with_centres_on_its_vertices_is_half_open(axis):
    dx = 2.0 ** -10
    org = np.array([3, -2, 5]) * dx
    tri = box_triangles(*[org[a] + np.array([1, 3, 4, 6]) * dx for a in range(3)])
    want = np.zeros((8, 8, 8), bool)
    want[1:6, 1:6, 1:6] = True
    got, leaks = _device(tri, org - dx / 2, dx, (8, 8, 8), axis)
    assert np.array_equal(got, want) and not np.any(leaks)


@pytest.mark.parametrize('seed', range(vr.VOX_FUZZ_SEEDS))
def test_fuzz_equals_the_cpu_statement(seed):
    kind, tri, org, dx, shape, axis = vr.fuzz_case(seed)
    _same(tri, org, dx, shape, axis, 'fuzz %d %s' % (seed, kind))
    if seed % 4 == 0:
        _same(tri, org, dx, shape, 'majority', 'fuzz %d %s' % (seed, kind))


def test_outside_clipped_degenerate_and_empty():
    dx, shape = 1e-3, (20, 17, 23)
    org = np.array([0.01, 0.02, -0.005])
    ext = np.array(shape) * dx
    for axis in AXES:
        # far outside, on every side and diagonal
        far = [box_triangles(*[org[a] + ext[a] * (0.5 + 40.0 * s[a]) + np.array([-2.0, 2.0]) * dx for a in range(3)])
               for s in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -1, -1))]
        got, leaks = _same(np.concatenate(far), org, dx, shape, axis, 'far outside')
        assert not got.any()
        # a box that sticks out of every side of the grid, and six that stick out of one side each
        _same(box_triangles(*[org[a] + np.array([-3.3, shape[a] + 2.6]) * dx for a in range(3)]), org, dx, shape, axis,
              'larger than the grid')
        for side in range(6):
            a, plus = side // 2, side % 2
            lines = [org[m] + np.array([3.2, shape[m] - 4.7]) * dx for m in range(3)]
            lines[a] = org[a] + (np.array([shape[a] - 5.1, shape[a] + 6.3]) if plus else np.array([-6.3, 5.1])) * dx
            got, _ = _same(box_triangles(*lines), org, dx, shape, axis, 'out of side %d' % side)
            assert got.any()
        # zero area (repeated vertex, collinear), zero projected area (a wall along each axis) next to a proper box
        inner = box_triangles(*[org[a] + np.array([4.4, 9.7]) * dx for a in range(3)])
        p = org + 7.3 * dx
        pz, d = np.round(p * 1024.0) / 1024.0, 2.0 ** -10       # collinear in doubles too, not a sliver after rounding
        junk = np.array([[p, p, p], [p, p, p + dx], [pz, pz + 2 * d, pz + 4 * d],
                         [p, p + np.array([0, dx, 0]), p + np.array([0, dx, 3 * dx])],
                         [p, p + np.array([dx, 0, 0]), p + np.array([3 * dx, 0, 2 * dx])],
                         [p, p + np.array([dx, 0, 0]), p + np.array([2 * dx, 5 * dx, 0])]])
        got, leaks = _device(np.concatenate([inner, junk[:3]]), org, dx, shape, axis)
        want, _ = _cpu(inner, org, dx, shape, axis)
        assert np.array_equal(got, want) and not np.any(leaks)
        _same(np.concatenate([inner, junk]), org, dx, shape, axis, 'degenerate')
        got, leaks = _device(np.zeros((0, 3, 3)), org, dx, shape, axis)
        assert got.shape == shape and not got.any() and not np.any(leaks)


def test_open_meshes_leak_as_the_cpu_statement_says():
    dx, shape = 1e-3, (30, 26, 34)
    org = np.array([0.0, 0.002, -0.001])
    cen = org + 0.5 * np.array(shape) * dx
    # the side of a tilted tube without caps, the ray along the tube as nearly as the grid has an axis for it
    side = tube_triangles(cen, (0.3, 0.2, 1.0), 0.012, 0.009, 23, 3)
    got, leaks = _same(side, org, dx, shape, 2, 'open tube')
    assert leaks > 0
    for axis in (0, 1):
        _same(side, org, dx, shape, axis, 'open tube')
    # a box with one side triangle removed: the majority repairs every column but those the CPU statement also reports
    lines = [org[a] + np.array([4.3, shape[a] - 5.6]) * dx for a in range(3)]
    box = box_triangles(*lines)
    closed, _ = _device(box, org, dx, shape, 'majority')
    for drop in (0, 5, 10):
        holed = np.delete(box, drop, axis=0)
        got, leaks = _same(holed, org, dx, shape, 'majority', 'box without triangle %d' % drop)
        assert sum(leaks) > 0 and sorted(leaks)[:2] == [0, 0]          # the hole faces one ray axis only
        assert np.array_equal(got, closed)                                # two sound axes outvote the leaking one
        a = int(np.argmax(leaks))
        one, leak1 = _same(holed, org, dx, shape, a, 'box without triangle %d' % drop)
        assert leak1 == leaks[a] and not np.array_equal(one, closed)


@pytest.mark.parametrize('shape', [(20, 24, 70), (70, 20, 24), (12, 416, 20), (18, 12, 416), (33, 64, 96)])
def test_columns_longer_than_one_word(shape):
    """more than one 32-voxel word per column, full and ragged last words, on every ray axis"""
    dx = 1e-3
    org = np.array([-0.004, 0.0011, 0.02])
    ext = np.array(shape) * dx
    tri, _, _ = vr.geodesic_polyhedron(org + 0.52 * ext, 0.47 * float(ext.max()), 1)
    tri2, _ = vr.closed_tube(org + 0.5 * ext, (0.2, 0.3, 1.0), 0.46 * float(ext.max()), 0.4 * float(np.sort(ext)[0]), 19, 2)
    for axis in AXES:
        _same(tri, org, dx, shape, axis, 'geodesic')
        got, _ = _same(tri2, org, dx, shape, axis, 'prism')
        assert got.any()


PRISM = dict(origin=np.array([0.0123, -0.004, 0.0007]), dx=1e-3, shape=(40, 36, 44), axis=(0.3, 0.2, 1.0), half=0.015,
             radius=0.011, rings=3)


def _closed_form(what, tri, org, dx, shape, dist, axes=AXES, share=1e-4):
    near = np.abs(dist) < 1e-9 * dx
    n_near = int(near.sum())
    assert n_near <= share * near.size, (what, n_near)
    inside = dist < 0
    for axis in axes:
        got, leaks = _device(tri, org, dx, shape, axis)
        bad = int((got != inside)[~near].sum())
        print('VOXELIZE closed form %s axis %s: %d solid, %d near cells left out (%.2e of the grid), %d mismatches'
              % (what, axis, int(inside.sum()), n_near, n_near / near.size, bad))
        assert bad == 0 and not np.any(leaks), (what, axis, bad, leaks)
    return n_near


@pytest.mark.parametrize('sections', [24, 64])
def test_tilted_prism_equals_the_closed_form(sections):
    p = PRISM
    cen = p['origin'] + 0.5 * np.array(p['shape']) * p['dx']
    tri, _ = vr.closed_tube(cen, p['axis'], p['half'], p['radius'], sections, p['rings'])
    dist = vr.prism_distance(p['origin'], p['dx'], p['shape'], cen, p['axis'], p['half'], p['radius'], sections)
    assert _closed_form('prism %d' % sections, tri, p['origin'], p['dx'], p['shape'], dist) == 0    # none near, as measured on the CPU


def test_geodesic_sphere_equals_its_half_spaces():
    org, dx, shape = np.array([-0.0031, 0.0102, 0.0]), 1e-3, (60, 66, 58)
    cen = org + np.array([30.2, 32.9, 28.1]) * dx
    tri, n, off = vr.geodesic_polyhedron(cen, 0.0265, 3)
    assert len(tri) == 1280
    _closed_form('geodesic 1280', tri, org, dx, shape, vr.polyhedron_distance(org, dx, shape, cen, n, off))
    lo = org + np.array([3.3, 2.2, 4.4]) * dx
    r = np.array([22.0, 27.5, 19.25]) * dx
    _closed_form('octahedron', vr.octahedron_triangles(lo + r, r), org, dx, shape, vr.octahedron_distance(org, dx, shape, lo + r, r))


def test_512_cubed_box_and_prism_equal_closed_forms():
    """the flagship size: the 12-triangle box (two triangles over 512 x 512 columns) and a 64-gon prism along z, against
    masks built on the host from the half-open box rule and the polygon's half planes"""
    import torch
    from adi_thermal_fields_amd.voxelize import voxelize_solid
    n, dx = 512, 1e-3
    org = np.array([0.0123, -0.004, 0.0007])
    idx = np.arange(n)
    lo, hi = np.array([3.3, 0.0, 17.25]), np.array([508.8, 512.0, 500.5])       # in voxels; one pair of sides on the grid's own
    box = box_triangles(*[org[a] + np.array([lo[a], hi[a]]) * dx for a in range(3)])
    inside1 = [(org[a] + (idx + 0.5) * dx >= org[a] + lo[a] * dx) & (org[a] + (idx + 0.5) * dx < org[a] + hi[a] * dx) for a in range(3)]
    want = inside1[0][:, None, None] & inside1[1][None, :, None] & inside1[2][None, None, :]
    for axis in AXES:
        got, leaks = voxelize_solid(vr_mesh(box), org, dx, (n, n, n), axis=axis, return_leaks=True, as_tensor=True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, n, n) and got.is_cuda
        bad = int((got.cpu().numpy().astype(bool) != want).sum())
        print('VOXELIZE 512^3 box axis %s: %d solid, %d mismatches, leaks %s' % (axis, int(want.sum()), bad, leaks))
        assert bad == 0 and not np.any(leaks)
    # prism along z: the closed form is a polygon test per column and an interval along z
    cen = org + np.array([255.7, 257.2, 256.0]) * dx
    half, radius, sections = 231.3 * dx, 243.6 * dx, 64
    tri, _ = vr.closed_tube(cen, (0.0, 0.0, 1.0), half, radius, sections, 5)
    d2 = vr.prism_distance(org, dx, (n, n, 1), cen - np.array([0.0, 0.0, cen[2] - org[2] - 0.5 * dx]), (0.0, 0.0, 1.0),
                           half, radius, sections)[:, :, 0]
    dz = np.abs(org[2] + (idx + 0.5) * dx - cen[2]) - half
    near = (np.abs(d2) < 1e-9 * dx)[:, :, None] | (np.abs(dz) < 1e-9 * dx)[None, None, :]
    n_near = int(near.sum())
    assert n_near <= 1e-4 * near.size, n_near
    want = (d2 < 0)[:, :, None] & (dz < 0)[None, None, :]
    for axis in AXES:
        got, leaks = voxelize_solid(vr_mesh(tri), org, dx, (n, n, n), axis=axis, return_leaks=True)
        bad = int((got != want)[~near].sum())
        print('VOXELIZE 512^3 prism axis %s: %d solid, %d near cells left out, %d mismatches, leaks %s'
              % (axis, int(want.sum()), n_near, bad, leaks))
        assert bad == 0 and not np.any(leaks)


def test_tensor_output_feeds_the_consumers():
    """as_tensor: a dense device uint8 mask that solidify_mask, STLBoundaryCorrector and Grid3D take as it is"""
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd.voxel_bc_correction import TriangleMesh, build_corrected_robin_fields
    from adi_thermal_fields_amd.voxel_morph import solidify_mask
    from adi_thermal_fields_amd.voxelize import voxel_grid_for, voxelize_solid
    p = PRISM
    cen = p['origin'] + 0.5 * np.array(p['shape']) * p['dx']
    mesh = TriangleMesh(vr.closed_tube(cen, p['axis'], p['half'], p['radius'], 24, p['rings'])[0])
    origin, shape = voxel_grid_for(mesh, p['dx'], pad=1.5 * p['dx'])
    t = voxelize_solid(mesh, origin, p['dx'], shape, as_tensor=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    host = voxelize_solid(mesh, origin, p['dx'], shape)
    assert np.array_equal(t.cpu().numpy().astype(bool), host) and host.any()
    assert not host[0].any() and not host[-1].any() and not host[:, :, 0].any()         # the pad is air
    assert torch.equal(solidify_mask(t, mode='auto'), t)                                 # a solid mask stays as it is
    base_h = {'x-': 25.0, 'x+': 25.0, 'z+': 40.0}
    r_dev, _ = build_corrected_robin_fields(mesh, t, origin, p['dx'], base_h)
    r_host, _ = build_corrected_robin_fields(mesh, host, origin, p['dx'], base_h)
    grid = hip.Grid3D(*shape, p['dx'], t)
    assert np.array_equal(grid.mask, host)
    for f in base_h:
        assert np.array_equal(grid.layout.to_host(r_dev[f]), r_host[f]), f
        assert np.count_nonzero(r_host[f]) > 0


def test_stl_file_to_three_steps(tmp_path):
    """STL (millimetres) -> load_voxel_from_stl_mm -> build_corrected_robin_fields -> three Cartesian steps; the mask is the
    closed-form one and the temperatures are those of the same three steps from the host-built mask"""
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd.voxel_bc_correction import build_corrected_robin_fields
    from adi_thermal_fields_amd.voxelize import load_voxel_from_stl_mm
    cen, axis, half, radius, sections = np.array([31.7, -4.2, 20.3]), (0.3, 0.2, 1.0), 15.0, 11.0, 24
    # vertices rounded to the file's float32 first, so the mesh in the file IS the mesh of the closed form's tolerance
    tri = vr.closed_tube(cen, axis, half, radius, sections, 3)[0].astype(np.float32).astype(np.float64)
    path = os.path.join(str(tmp_path), 'prism.stl')
    vr.write_binary_stl(path, tri)
    mask, origin_mm, dx_mm, shape, mesh = load_voxel_from_stl_mm(path, 1.0, pad_mm=1.5)
    assert isinstance(mask, np.ndarray) and mask.dtype == np.bool_ and mask.shape == shape and dx_mm == 1.0
    assert np.array_equal(mesh.triangles, tri)
    lo = tri.reshape(-1, 3).min(axis=0)
    assert np.array_equal(np.asarray(origin_mm), lo - 1.5)
    assert shape == tuple(int(np.ceil(e + 3.0)) for e in tri.reshape(-1, 3).max(axis=0) - lo)
    dist = vr.prism_distance(origin_mm, dx_mm, shape, cen, axis, half, radius, sections)
    # float32 vertices move the surface by up to 2^-24 * 64 mm: cells nearer than that are left out, and counted
    near = np.abs(dist) < 1e-5
    assert near.sum() <= 1e-4 * near.size
    want = dist < 0
    assert np.array_equal(mask[~near], want[~near]) and 9000 < mask.sum() < 13000
    want = np.where(near, mask, want)                       # the host-built mask, the near cells (if any) as voxelised
    # auto_dx: the same file under a voxel budget
    m2, o2, dx2, s2, _ = load_voxel_from_stl_mm(path, 1.0, pad_mm=1.5, max_voxels=20000)
    n0 = shape[0] * shape[1] * shape[2]
    assert dx2 == 1.0 * (n0 / 20000.0) ** (1.0 / 3.0) and m2.shape == s2 and s2[0] * s2[1] * s2[2] < 1.2 * 20000
    assert abs(m2.mean() - mask.mean()) < 0.02

    mat = dict(cases.STEEL)
    dx = dx_mm * 1e-3
    base_h = {'x-': 25.0, 'x+': 25.0, 'y+': 10.0, 'z-': 300.0, 'z+': 40.0}
    rng = np.random.default_rng(4)
    T0 = np.where(want, rng.uniform(20.0, 1000.0, shape), 20.0)
    dt = 40.0 * dx * dx / (mat['k'] / (mat['rho'] * mat['cp']))

    def three_steps(m):
        robin, _ = build_corrected_robin_fields(mesh, m, origin_mm, dx_mm, base_h)
        grid = hip.Grid3D(*shape, dx, m)
        packs = hip.precompute_coeff_packs_unified(grid, hip.Material(**mat), robin_h=robin)
        T = T0
        for _ in range(3):
            T = hip.adi_step_numba_coeff(T, grid, hip.Material(**mat), hip.Params(dt, 0.5), packs, Tinf=20.0)
        return np.asarray(T)
    got, ref = three_steps(mask), three_steps(want)
    e = rel_linf(got, ref)
    print('VOXELIZE end to end: %d solid cells, rel_linf %.3e after three steps' % (int(mask.sum()), e))
    assert e == 0.0
    assert np.abs(ref - T0).max() > 1.0
