"""CPU: the yardstick of the voxeliser tests (tests/voxelize_ref.py) and the host parts of
adi_thermal_fields_amd.voxelize.

The GPU tests compare the device mask with the NumPy statement of the definition bit for bit, so the statement itself is
pinned here: against exact rational arithmetic where every operation is exact, against masks turned into their own
surface, and against a closed-form inside test.
"""
import ctypes
import math

import numpy as np
import pytest

import voxelize_ref as vr
from stlcorr_meshes import box_triangles, plate_triangles


@pytest.mark.parametrize('case', vr.dyadic_cases(), ids=lambda c: c[0])
def test_fp64_statement_equals_rational_arithmetic(case):
    name, tri, org, dx, shape = case
    assert max(shape) <= 16 + 1 and dx == 2.0 ** -10
    assert np.all(np.round(tri / (dx / 8)) * (dx / 8) == tri) and np.all(np.round(org / (dx / 8)) * (dx / 8) == org)
    for axis in range(3):
        got, leak = vr.voxelize(tri, org, dx, shape, axis)
        want, leak_x = vr.voxelize_exact(tri, org, dx, shape, axis)
        assert np.array_equal(got, want), (name, axis, int((got != want).sum()))
        assert leak == leak_x == 0, (name, axis, leak, leak_x)
        assert got.any()


def test_clipping_to_the_bounding_box_changes_nothing():
    """the device tests only the columns of a triangle's bounding box; so does voxelize(clip=True)"""
    cases = [c[1:] + (a,) for c in vr.dyadic_cases()[:4] for a in range(3)]
    cases += [vr.fuzz_case(s)[1:] for s in range(vr.VOX_FUZZ_SEEDS) if np.prod(vr.fuzz_case(s)[4]) * len(vr.fuzz_case(s)[1]) < 4e7]
    assert len(cases) >= 20
    for tri, org, dx, shape, axis in cases:
        a, la = vr.voxelize(tri, org, dx, shape, axis, clip=True)
        b, lb = vr.voxelize(tri, org, dx, shape, axis, clip=False)
        assert np.array_equal(a, b) and la == lb


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_mask_to_surface_to_mask(axis):
    rng = np.random.default_rng(3)
    shape, dx = (9, 7, 11), 2.0 ** -10
    mask = rng.random(shape) >= 0.35
    for org in (np.array([3, -2, 5]) * dx, np.array([0.0123, -0.004, 0.0007])):
        tri = plate_triangles(mask, [org[a] + np.arange(shape[a] + 1) * dx for a in range(3)])
        got, leak = vr.voxelize(tri, org, dx, shape, axis)
        assert np.array_equal(got, mask) and leak == 0
        # every centre on a mesh plane, edge or vertex: behind the surface, so the mask moves by one voxel
        got, leak = vr.voxelize(tri, org - dx / 2, dx, tuple(s + 1 for s in shape), axis)
        assert np.array_equal(got[:-1, :-1, :-1], mask) and leak == 0
        assert not got[-1].any() and not got[:, -1].any() and not got[:, :, -1].any()


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_cut_box_with_centres_on_its_vertices_is_half_open(axis):
    dx = 2.0 ** -10
    org = np.array([3, -2, 5]) * dx
    tri = box_triangles(*[org[a] + np.array([1, 3, 4, 6]) * dx for a in range(3)])
    want = np.zeros((8, 8, 8), bool)
    want[1:6, 1:6, 1:6] = True
    got, leak = vr.voxelize(tri, org - dx / 2, dx, (8, 8, 8), axis)
    assert np.array_equal(got, want) and leak == 0


PRISM = dict(origin=np.array([0.0123, -0.004, 0.0007]), dx=1e-3, shape=(40, 36, 44), axis=(0.3, 0.2, 1.0), half=0.015,
             radius=0.011, rings=3)


@pytest.mark.parametrize('sections', [24, 64])
def test_tilted_prism_equals_the_closed_form(sections):
    p = PRISM
    cen = p['origin'] + 0.5 * np.array(p['shape']) * p['dx']
    tri, _ = vr.closed_tube(cen, p['axis'], p['half'], p['radius'], sections, p['rings'])
    dist = vr.prism_distance(p['origin'], p['dx'], p['shape'], cen, p['axis'], p['half'], p['radius'], sections)
    near = np.abs(dist) < 1e-9 * p['dx']
    assert int(near.sum()) == 0
    res = []
    for axis in range(3):
        got, leak = vr.voxelize(tri, p['origin'], p['dx'], p['shape'], axis)
        assert leak == 0
        assert int((got != (dist < 0)).sum()) == 0, (sections, axis)
        res.append(got)
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[1], res[2])
    assert 10000 < int(res[0].sum()) < 12500


def test_geodesic_polyhedron_is_convex_and_voxelises_to_its_half_spaces():
    org, dx, shape = np.array([-0.0031, 0.0102, 0.0]), 1e-3, (30, 34, 28)
    cen = org + np.array([15.2, 16.9, 14.1]) * dx
    tri, n, off = vr.geodesic_polyhedron(cen, 0.0125, 2)
    assert len(tri) == 320
    # convex: every vertex on or behind every face plane
    worst = max(float(np.max((tri.reshape(-1, 3) - cen) @ nn - oo)) for nn, oo in zip(n, off))
    assert worst < 1e-12 * 0.0125
    dist = vr.polyhedron_distance(org, dx, shape, cen, n, off)
    near = np.abs(dist) < 1e-9 * dx
    assert near.sum() <= 1e-4 * dist.size
    for axis in range(3):
        got, leak = vr.voxelize(tri, org, dx, shape, axis)
        assert leak == 0 and np.array_equal(got[~near], (dist < 0)[~near])


def test_open_meshes_leak():
    from stlcorr_meshes import tube_triangles
    org, dx, shape = np.array([0.0, 0.0, 0.0]), 1e-3, (20, 20, 24)
    side = tube_triangles(org + 0.5 * np.array(shape) * dx, (0.0, 0.0, 1.0), 0.008, 0.007, 17, 2)
    _, leak = vr.voxelize(side, org, dx, shape, 2)          # the ray along the tube: nothing is crossed, nothing leaks
    assert leak == 0
    side = tube_triangles(org + 0.5 * np.array(shape) * dx, (0.3, 0.2, 1.0), 0.008, 0.007, 17, 2)
    _, leak = vr.voxelize(side, org, dx, shape, 2)
    assert leak > 0


def test_voxel_grid_for():
    from adi_thermal_fields_amd.voxelize import voxel_grid_for
    tri = np.array([[[1.0, 2.0, -1.0], [3.0, 2.5, -1.0], [1.0, 4.0, 0.25]]])
    origin, shape = voxel_grid_for(tri, 0.5)
    assert origin.tolist() == [1.0, 2.0, -1.0] and shape == (4, 4, 3)      # 2 / 0.5 whole, 2 / 0.5, ceil(1.25 / 0.5)
    origin, shape = voxel_grid_for(tri, 0.5, pad=0.25)
    assert origin.tolist() == [0.75, 1.75, -1.25] and shape == (5, 5, 4)
    origin, shape = voxel_grid_for(tri, 0.75)
    assert shape == (3, 3, 2)                                              # ceil(2.67), ceil(2.67), ceil(1.67)
    flat = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    assert voxel_grid_for(flat, 0.25)[1] == (4, 4, 1)                      # never an empty axis
    mesh = type('M', (), {'triangles': tri})()
    assert voxel_grid_for(mesh, 0.5)[1] == (4, 4, 3)
    with pytest.raises(ValueError):
        voxel_grid_for(tri, 0.0)
    with pytest.raises(ValueError):
        voxel_grid_for(np.zeros((0, 3, 3)), 0.5)


def test_voxelize_calls_reject_bad_arguments_without_gpu():
    """validation comes before any HIP call"""
    from adi_thermal_fields_amd import _lib
    lib, check, p = _lib.lib, _lib.check, ctypes.c_void_p(256)
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    n = ctypes.c_long(-7)
    check(lib.adi_voxelize_words(512, 512, 512, 2, ctypes.byref(n)))
    assert n.value == 17 * 512 * 512
    check(lib.adi_voxelize_words(70, 3, 5, 0, ctypes.byref(n)))
    assert n.value == 3 * 15
    check(lib.adi_voxelize_words(64, 3, 5, 0, ctypes.byref(n)))
    assert n.value == 3 * 15                                  # 64 voxels and the bit behind them
    for axis in (-1, 3):
        with pytest.raises(ValueError, match='ray axis'):
            check(lib.adi_voxelize_words(4, 4, 4, axis, ctypes.byref(n)))
        with pytest.raises(ValueError, match='ray axis'):
            check(lib.adi_voxelize_count(p, 1, org, 1e-3, 4, 4, 4, axis, p, None))
        with pytest.raises(ValueError, match='ray axis'):
            check(lib.adi_voxelize_toggle(p, p, 1, 1, org, 1e-3, 4, 4, 4, axis, p, None))
        with pytest.raises(ValueError, match='ray axis'):
            check(lib.adi_voxelize_scan(p, 4, 4, 4, axis, p, p, None))
    for dx in (0.0, -1e-3, float('nan')):
        with pytest.raises(ValueError, match='dx must be positive'):
            check(lib.adi_voxelize_count(p, 1, org, dx, 4, 4, 4, 0, p, None))
        with pytest.raises(ValueError, match='dx must be positive'):
            check(lib.adi_voxelize_toggle(p, p, 1, 1, org, dx, 4, 4, 4, 0, p, None))
    for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        with pytest.raises(ValueError, match='bad grid'):
            check(lib.adi_voxelize_words(*shape, 1, ctypes.byref(n)))
        with pytest.raises(ValueError, match='bad grid'):
            check(lib.adi_voxelize_count(p, 1, org, 1e-3, *shape, 1, p, None))
        with pytest.raises(ValueError, match='bad grid'):
            check(lib.adi_voxelize_toggle(p, p, 1, 1, org, 1e-3, *shape, 1, p, None))
        with pytest.raises(ValueError, match='bad grid'):
            check(lib.adi_voxelize_scan(p, *shape, 1, p, p, None))
    with pytest.raises(ValueError, match='bad triangle count'):
        check(lib.adi_voxelize_count(p, -1, org, 1e-3, 4, 4, 4, 0, p, None))
    with pytest.raises(ValueError, match='bad triangle count'):
        check(lib.adi_voxelize_toggle(p, p, -1, 0, org, 1e-3, 4, 4, 4, 0, p, None))
    with pytest.raises(ValueError, match='bad tile count'):
        check(lib.adi_voxelize_toggle(p, p, 1, -1, org, 1e-3, 4, 4, 4, 0, p, None))
    with pytest.raises(ValueError, match='without a triangle'):
        check(lib.adi_voxelize_toggle(p, p, 0, 5, org, 1e-3, 4, 4, 4, 0, p, None))
    with pytest.raises(ValueError, match='null origin'):
        check(lib.adi_voxelize_count(p, 1, None, 1e-3, 4, 4, 4, 0, p, None))
    with pytest.raises(ValueError, match='null argument'):
        check(lib.adi_voxelize_scan(None, 4, 4, 4, 0, p, p, None))
    with pytest.raises(ValueError, match='16-byte aligned'):
        check(lib.adi_voxelize_scan(p, 4, 4, 4, 0, ctypes.c_void_p(264), p, None))
    with pytest.raises(ValueError, match='null argument'):
        check(lib.adi_voxelize_majority(p, p, None, 64, p, None))
    # nothing to do is not an error and launches nothing
    check(lib.adi_voxelize_count(None, 0, org, 1e-3, 4, 4, 4, 0, None, None))
    check(lib.adi_voxelize_toggle(None, None, 0, 0, org, 1e-3, 4, 4, 4, 0, None, None))
    check(lib.adi_voxelize_majority(None, None, None, 0, None, None))


def test_public_arguments_are_checked_before_the_gpu_is_needed():
    from adi_thermal_fields_amd.voxelize import load_voxel_from_stl_mm, voxelize_solid
    tri = np.zeros((1, 3, 3))
    with pytest.raises(ValueError, match='dx must be positive'):
        voxelize_solid(tri, (0, 0, 0), 0.0, (4, 4, 4))
    with pytest.raises(ValueError, match='bad grid shape'):
        voxelize_solid(tri, (0, 0, 0), 1.0, (4, 0, 4))
    with pytest.raises(ValueError, match='axis must be'):
        voxelize_solid(tri, (0, 0, 0), 1.0, (4, 4, 4), axis=3)
    with pytest.raises(NotImplementedError, match='subdivide'):
        load_voxel_from_stl_mm('no_such_file.stl', 1.0, voxel_method='subdivide')
