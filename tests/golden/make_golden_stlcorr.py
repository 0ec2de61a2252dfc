#!/usr/bin/env python3
"""Golden vectors of the reference's STL correction of voxel Robin coefficients -- /root/reference/voxel_bc_correction.py
(STLBoundaryCorrector.compute_voxel_projected_areas / build_corrected_fields) -- produced by IMPORTING THE REFERENCE in the
build container (it never travels; tests/golden/stlcorr_*.npz do).

    python tests/golden/make_golden_stlcorr.py

The module never imports trimesh: it reads `triangles`, `triangles_center`, `face_normals` and `area_faces` from the mesh
object, so it is driven here with a plain namespace holding those arrays for meshes built by formula (tilted cylinder,
tilted conical frustum, a finely tessellated tube).  Normals and areas are computed the way trimesh does (cross product of
the edge vectors, its norm).  Every file holds: triangles, normals, areas, mask, origin, dx, max_subdiv, area_epsilon, the
faces and values of base_h, the reference's robin / scale fields with and without the fallback (`robin_on_<face>`,
`scale_on_<face>`, `robin_off_<face>`, `scale_off_<face>`), the six projected-area fields (`area_<face>`), the number of
contributions per voxel face (`count`, face-major) and its maximum `n_max`.

Two groups (`python tests/golden/make_golden_stlcorr.py [margin|boundary|all]`, default all).

margin: asserted on every case, so that the reference's own binning does not hang on the last bit of a rounding: no centroid
component lies within 1e-9 dx of a voxel boundary, and no span_max at or below max_subdiv lies within 1e-9 of an integer.

boundary: the opposite.  Planar faces ON voxel planes (a part drawn in millimetres), spans that are whole numbers of
voxels, normals at the 1e-12 tolerance, NaN / huge / subnormal inputs: the voxel of a sub-triangle is whatever IEEE
arithmetic in NumPy's order gives.  Asserted per case: at least `boundary_share_min` of all centroid components lie within
4 ulp of a voxel boundary (exactly on it included); the measured share is stored as `boundary_share`, the share exactly on
a boundary as `boundary_share_exact`.

Also printed: the reference's CPU time per sub-triangle in this container (DESIGN.md section 6d quotes it).
"""
import math
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(HERE))

import voxel_bc_correction as ref  # noqa: E402
import stlcorr_meshes as sm  # noqa: E402

GROUP = sys.argv[1] if len(sys.argv) > 1 else 'all'
assert GROUP in ('margin', 'boundary', 'all'), GROUP

FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')


# ---- meshes by formula ----------------------------------------------------------------------------------------------
def _frame(axis):
    u = np.asarray(axis, dtype=float)
    u = u / np.linalg.norm(u)
    a = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, a)
    e1 /= np.linalg.norm(e1)
    return u, e1, np.cross(u, e1)


def frustum_triangles(centre, axis, half_len, r_lo, r_hi, sections, caps=True, rings=1, phase=0.0):
    """closed (caps=True) cone frustum about `axis`: `sections` x `rings` side quads split in two, one fan triangle per
    section and cap; outward winding.  r_lo == r_hi gives a cylinder."""
    u, e1, e2 = _frame(axis)
    c = np.asarray(centre, dtype=float)
    th = phase + 2.0 * math.pi * np.arange(sections + 1) / sections
    ring = lambda s: (c + (2.0 * s - 1.0) * half_len * u
                      + (r_lo + (r_hi - r_lo) * s) * (np.cos(th)[:, None] * e1 + np.sin(th)[:, None] * e2))
    tris = []
    for m in range(rings):
        lo, hi = ring(m / rings), ring((m + 1) / rings)
        for k in range(sections):
            tris.append((lo[k], lo[k + 1], hi[k + 1]))
            tris.append((lo[k], hi[k + 1], hi[k]))
    if caps:
        lo, hi = ring(0.0), ring(1.0)
        c_lo, c_hi = c - half_len * u, c + half_len * u
        for k in range(sections):
            tris.append((c_lo, lo[k + 1], lo[k]))
            tris.append((c_hi, hi[k], hi[k + 1]))
    return np.array(tris, dtype=np.float64)


def frustum_mask(shape, origin, dx, centre, axis, half_len, r_lo, r_hi):
    """voxels whose centre lies inside the frustum"""
    u, _, _ = _frame(axis)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'), axis=-1)
    p = np.asarray(origin) + (idx + 0.5) * dx - np.asarray(centre)
    t = p @ u
    rad = np.linalg.norm(p - t[..., None] * u, axis=-1)
    s = (t / half_len + 1.0) * 0.5
    return (np.abs(t) <= half_len) & (rad <= r_lo + (r_hi - r_lo) * s)


def mesh_of(tri):
    """the four arrays of a trimesh.Trimesh, computed as trimesh computes them"""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    norm = np.linalg.norm(cross, axis=1) if len(tri) else np.zeros(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        normals = np.where(norm[:, None] > 0.0, cross / norm[:, None], 0.0)
    return types.SimpleNamespace(triangles=tri, triangles_center=tri.mean(axis=1) if len(tri) else np.zeros((0, 3)),
                                 face_normals=normals.reshape(-1, 3), area_faces=norm / 2.0)


# ---- the condition on the fixtures ----------------------------------------------------------------------------------
def check_margins(mesh, origin, dx, max_subdiv, area_epsilon):
    """-> (sub-triangles, smallest distance of a centroid component to a voxel boundary in dx, smallest distance of a
    span_max <= max_subdiv to an integer); arithmetic of the reference (its own _subdivide_triangle)"""
    nsub, dmin, smin = 0, 1.0, 1.0
    for t in range(len(mesh.triangles)):
        if float(mesh.area_faces[t]) <= area_epsilon:
            continue
        v = mesh.triangles[t]
        span_max = float(np.max((v.max(axis=0) - v.min(axis=0)) / dx))
        if span_max <= max_subdiv:
            smin = min(smin, abs(span_max - round(span_max)))
        n = int(math.ceil(span_max)) if span_max > 1.0 else 1
        n = max(1, min(n, max_subdiv))
        subs = (v,) if n == 1 else ref._subdivide_triangle(v, n)
        assert len(subs) == n * n
        for s in subs:
            q = (np.mean(s, axis=0) - origin) / dx
            dmin = min(dmin, float(np.min(np.abs(q - np.round(q)))))
        nsub += len(subs)
    assert dmin > 1e-9, 'a centroid lies %.3e dx from a voxel boundary' % dmin
    assert smin > 1e-9, 'a span_max lies %.3e from an integer' % smin
    return nsub, dmin, smin


def boundary_share(mesh, origin, dx, max_subdiv, area_epsilon):
    """-> (sub-triangles, share of the finite centroid components within 4 ulp of a voxel boundary, share exactly on one);
    arithmetic of the reference"""
    nsub, comps, near, exact = 0, 0, 0, 0
    for t in range(len(mesh.triangles)):
        if float(mesh.area_faces[t]) <= area_epsilon:
            continue
        v = mesh.triangles[t]
        with np.errstate(invalid='ignore', over='ignore'):
            span_max = float(np.max((v.max(axis=0) - v.min(axis=0)) / dx))
            n = int(math.ceil(span_max)) if span_max > 1.0 else 1
            n = max(1, min(n, max_subdiv))
            subs = (v,) if n == 1 else ref._subdivide_triangle(v, n)
            q = (np.array([np.mean(s, axis=0) for s in subs]) - origin) / dx
            fin = np.isfinite(q)
            d = np.abs(q[fin] - np.round(q[fin]))
            near += int(np.count_nonzero(d <= 4.0 * np.spacing(np.maximum(np.abs(q[fin]), 1.0))))
        exact += int(np.count_nonzero(d == 0.0))
        comps += int(fin.sum())
        nsub += len(subs)
    return nsub, near / max(comps, 1), exact / max(comps, 1)


# ---- one case -------------------------------------------------------------------------------------------------------
def dense(projected, shape):
    area = {f: np.zeros(shape) for f in FACES}
    for idx, vdata in projected.items():
        for f, a in vdata.projected_area.items():
            area[f][idx] = a
    return area


def make(name, tri, mask, origin, dx, base_h, max_subdiv=6, area_epsilon=1e-16, share_min=None):
    """share_min None: a margin case (tri = vertices); else a boundary case (tri = a mesh namespace or vertices)"""
    mesh = mesh_of(tri) if share_min is None else (tri if hasattr(tri, 'triangles') else sm.mesh_of(tri))
    origin = np.asarray(origin, dtype=float)
    extra = {}
    if share_min is None:
        nsub, dmin, smin = check_margins(mesh, origin, dx, max_subdiv, area_epsilon)
    else:
        nsub, share, exact = boundary_share(mesh, origin, dx, max_subdiv, area_epsilon)
        assert share >= share_min, '%s: %.4f of the centroid components at a voxel boundary, below %.2f' % (
            name, share, share_min)
        extra = dict(boundary_share=np.float64(share), boundary_share_exact=np.float64(exact),
                     boundary_share_min=np.float64(share_min))
        dmin, smin = share, exact
    corr = ref.STLBoundaryCorrector(mesh, mask, origin, dx, max_subdiv=max_subdiv, area_epsilon=area_epsilon)

    counts = np.zeros((6,) + mask.shape, dtype=np.uint16)
    plain_add = ref.VoxelBoundaryData.add_projected_area

    def counting_add(self, face, area):
        if not area <= 0.0:                        # what add_projected_area lets through (a NaN too)
            counts[(FACES.index(face),) + self.voxel_index] += 1
        plain_add(self, face, area)
    ref.VoxelBoundaryData.add_projected_area = counting_add
    try:
        t0 = time.perf_counter()
        projected = corr.compute_voxel_projected_areas()
        dt = time.perf_counter() - t0
    finally:
        ref.VoxelBoundaryData.add_projected_area = plain_add
    t0 = time.perf_counter()
    corr.compute_voxel_projected_areas()
    dt_plain = time.perf_counter() - t0

    out = dict(extra, triangles=mesh.triangles, normals=mesh.face_normals, areas=mesh.area_faces, mask=mask, origin=origin,
               dx=np.float64(dx), max_subdiv=np.int64(max_subdiv), area_epsilon=np.float64(area_epsilon),
               base_faces=np.array(list(base_h.keys())), base_vals=np.array([float(v) for v in base_h.values()]),
               count=counts, n_max=np.int64(counts.max()), n_sub=np.int64(nsub))
    for f, a in dense(projected, mask.shape).items():
        out['area_' + f] = a
    for tag, fb in (('on', True), ('off', False)):
        robin, scale = corr.build_corrected_fields(base_h, fallback_to_base=fb)
        assert list(robin) == list(base_h) and list(scale) == list(base_h)
        for f in base_h:
            out['robin_%s_%s' % (tag, f)] = robin[f]
            out['scale_%s_%s' % (tag, f)] = scale[f]
    path = os.path.join(HERE, 'stlcorr_%s.npz' % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 800000, (name, size)
    what = ('margins %.1e dx / %.1e' if share_min is None
            else 'at a boundary (4 ulp) %.4f / exactly on one %.4f of the centroid components') % (dmin, smin)
    print('%-20s %5d triangles %7d sub-triangles, %6d voxels hit, n_max %3d, %s, '
          'reference %.2f s = %.1f us per sub-triangle, %d bytes'
          % (name, len(mesh.triangles), nsub, len(projected), counts.max(), what, dt_plain,
             1e6 * dt_plain / max(nsub, 1), size), flush=True)
    return nsub, dt_plain


SHAPE, DX = (40, 44, 48), 1.0e-3
H6 = {'x-': 400.0, 'x+': 37.5, 'y-': 410.0, 'y+': 999.0, 'z-': 12.25, 'z+': 500.0}
AXIS = (0.3, 0.2, 1.0)
CENTRE = (20.13e-3, 22.21e-3, 24.07e-3)
total = [0, 0.0]


def add(r):
    total[0] += r[0]
    total[1] += r[1]


def margin_group():
    # tilted cylinder, mask = the analytic voxelisation of the same cylinder; 64 sections: every triangle is cut 6 x 6
    cyl = dict(centre=CENTRE, axis=AXIS, half_len=14.03e-3, r_lo=11.02e-3, r_hi=11.02e-3)
    cyl_mask = frustum_mask(SHAPE, (0.0, 0.0, 0.0), DX, **cyl)
    add(make('cyl64', frustum_triangles(sections=64, **cyl), cyl_mask, (0.0, 0.0, 0.0), DX, H6))
    add(make('cyl700', frustum_triangles(sections=700, **cyl), cyl_mask, (0.0, 0.0, 0.0), DX, H6))

    # tilted conical frustum; base_h of five faces (no 'z+'), one of them zero
    fr = dict(centre=CENTRE, axis=(-0.25, 0.4, 1.0), half_len=13.01e-3, r_lo=12.03e-3, r_hi=5.04e-3)
    add(make('frustum', frustum_triangles(sections=96, **fr), frustum_mask(SHAPE, (0.0, 0.0, 0.0), DX, **fr), (0.0, 0.0, 0.0), DX,
             {'y+': 250.0, 'x-': 80.0, 'z-': 0.0, 'x+': 33.0, 'y-': 120.5}))

    # non-zero origin, the mesh partly outside the grid, two triangles too small to count and one AT area_epsilon (the
    # threshold is set to that triangle's area), max_subdiv 1 and 3
    ORG = (-3.2e-3, 1.7e-3, 0.4e-3)
    off = dict(centre=(3.11e-3, 24.3e-3, 40.2e-3), axis=(1.0, 0.35, 0.5), half_len=12.04e-3, r_lo=9.03e-3, r_hi=7.02e-3)
    off_tri = frustum_triangles(sections=80, **off)
    tiny = np.array([[[5e-3, 20e-3, 20e-3], [5e-3 + 2e-9, 20e-3, 20e-3], [5e-3, 20e-3 + 3e-9, 20e-3]],
                     [[8e-3, 25e-3, 30e-3], [8e-3, 25e-3 + 1e-9, 30e-3], [8e-3, 25e-3, 30e-3 + 1e-9]]])
    off_tri = np.concatenate([off_tri[:50], tiny[:1], off_tri[50:], tiny[1:]])
    off_mask = frustum_mask(SHAPE, ORG, DX, **off)
    eps_at = float(mesh_of(off_tri).area_faces[162])      # a triangle of the small cap: the smallest real area
    assert (mesh_of(off_tri).area_faces <= eps_at).sum() >= 3
    add(make('offgrid_sub1', off_tri, off_mask, ORG, DX, H6, max_subdiv=1, area_epsilon=eps_at))
    add(make('offgrid_sub3', off_tri, off_mask, ORG, DX, H6, max_subdiv=3, area_epsilon=eps_at))

    # an empty mesh: with the fallback every exposed face gets the base value, without it nothing
    add(make('empty', np.zeros((0, 3, 3)), cyl_mask, (0.0, 0.0, 0.0), DX, H6))

    # small triangles (the n == 1 branch): the side of a tilted tube in 0.45 mm x 0.47 mm quads
    tube = dict(centre=CENTRE, axis=AXIS, half_len=8.02e-3, r_lo=7.03e-3, r_hi=7.03e-3)
    small_tri = frustum_triangles(sections=98, caps=False, rings=34, phase=0.013, **tube)
    m = mesh_of(small_tri)
    assert float(np.max((m.triangles.max(axis=1) - m.triangles.min(axis=1)) / DX)) <= 1.0
    add(make('small', small_tri, frustum_mask(SHAPE, (0.0, 0.0, 0.0), DX, **tube), (0.0, 0.0, 0.0), DX, H6))


def boundary_group():
    shape = (24, 20, 28)
    lo, hi = np.array([3, 4, 5]), np.array([20, 16, 23])
    inside = np.zeros(shape, bool)
    inside[3:20, 4:16, 5:23] = True

    # an axis-aligned box on voxel planes, vertices written k * 1e-3 (a millimetre STL times scale=1e-3): not
    # representable, so (k * 1e-3 - 0) / 1e-3 is k or the number below it.  Sides in quads of about six voxels, max_subdiv 6;
    # one quad per side, max_subdiv 32 (n = 18 or 19)
    mm = lambda ks: [k * 1e-3 for k in ks]
    add(make('box_on_planes_sub6', sm.box_triangles(mm([3, 9, 14, 20]), mm([4, 10, 16]), mm([5, 11, 17, 23])), inside,
             (0.0, 0.0, 0.0), 1e-3, H6, max_subdiv=6, share_min=0.05))
    add(make('box_on_planes_sub32', sm.box_triangles(mm([3, 20]), mm([4, 16]), mm([5, 23])), inside, (0.0, 0.0, 0.0), 1e-3,
             H6, max_subdiv=32, share_min=0.05))

    # the same box through float32 millimetres times 1e-3 (what load_stl(path, scale=1e-3) gives), voxels of half a mm
    f32 = lambda ks: np.array([0.5 * k for k in ks], dtype=np.float32).astype(np.float64) * 1e-3
    add(make('box_f32_mm', sm.box_triangles(f32([3, 20]), f32([4, 16]), f32([5, 23])), inside, (0.0, 0.0, 0.0), 5e-4, H6,
             max_subdiv=40, share_min=0.05))

    # a non-zero origin with a negative component, the box shifted with it and partly outside the grid: floor of a
    # negative quotient (a truncation would fold voxel -1 into voxel 0) and of one past the last voxel
    org = np.array([-3.2e-3, 1.7e-3, 0.4e-3])
    at = lambda a, ks: [org[a] + k * 1e-3 for k in ks]
    part = np.zeros(shape, bool)
    part[0:10, 2:20, 3:20] = True
    add(make('box_shifted_origin', sm.box_triangles(at(0, [-3, 1, 5, 10]), at(1, [2, 8, 14, 19, 25]), at(2, [3, 9, 14, 20])),
             part, org, 1e-3, H6, max_subdiv=6, share_min=0.05))

    # a plate two voxels thick with through-holes, its surface as unit quads on the voxel planes: hits next to off-mask
    # drops, spans of one voxel up to rounding (n = 1 or 2); base_h: all distinct, one zero, one negative, 'z-' absent
    plate = np.zeros(shape, bool)
    plate[2:22, 2:18, 10:12] = True
    plate[5:8, 5:9, :] = False
    plate[12:17, 6:8, :] = False
    plate[10:11, 12:16, :] = False
    planes = [[k * 1e-3 for k in range(n + 1)] for n in shape]
    add(make('plate_with_holes', sm.plate_triangles(plate, planes), plate, (0.0, 0.0, 0.0), 1e-3,
             {'x-': 400.0, 'x+': -37.5, 'y-': 0.0, 'y+': 999.0, 'z+': 12.25}, max_subdiv=6, share_min=0.05))

    # deep cuts: a dozen large tilted triangles with vertices on the dyadic grid dx/8, dx = 2^-10 (spans are exact), cut up
    # to 46 x 46; one that spans 80 voxels (clamped to max_subdiv = 64) and leaves the grid; spans of exactly 1.0, 2.0 and
    # 6.0 voxels (`> 1.0`, ceil at an integer)
    dxd = 2.0 ** -10
    rng = np.random.default_rng(64)
    big = []
    while len(big) < 12:
        t = rng.integers(2 * 8, 46 * 8, (3, 3)) / 8.0
        if 20.0 <= (t.max(axis=0) - t.min(axis=0)).max() and np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) > 300.0:
            big.append(t)
    exact = [[[10, 10, 10], [11, 10.5, 10.25], [10.5, 11, 10.75]], [[20, 20, 20], [22, 21, 20.5], [21, 22, 21.5]],
             [[30, 10, 10], [36, 12, 13], [33, 16, 11]], [[-20, 5, 7], [60, 30, 20], [10, 44, 40]]]
    deep = np.array(big + exact, dtype=np.float64) * dxd
    spans = ((deep.max(axis=1) - deep.min(axis=1)) / dxd).max(axis=1)
    assert spans[12:].tolist() == [1.0, 2.0, 6.0, 80.0] and spans[:12].max() <= 64.0, spans
    idx = np.stack(np.meshgrid(*[np.arange(48)] * 3, indexing='ij'), axis=-1)
    ball = ((idx + 0.5 - 24.0) ** 2).sum(axis=-1) <= 22.0 ** 2
    add(make('deep_subdiv', deep, ball, (0.0, 0.0, 0.0), dxd, H6, max_subdiv=64, share_min=0.0))

    # normals at the tolerance of the projection: a component of exactly 1e-12, the doubles next to it on either side, 0,
    # and their negatives, on each axis in turn; hand-set (the reference reads face_normals, it does not recompute them)
    tol = 1e-12
    vals = [tol, np.nextafter(tol, 1.0), np.nextafter(tol, 0.0), 0.0, -tol, -np.nextafter(tol, 1.0), -np.nextafter(tol, 0.0),
            -0.0]
    tri, nrm = [], []
    for m, v in enumerate(vals):
        for ax in range(3):
            p = np.array([1.3 + m, 1.2 + 2 * ax + (m % 2), 2.4 + ax]) * 1e-3
            tri.append([p, p + [0.3e-3, 0.0, 0.1e-3], p + [0.0, 0.3e-3, 0.2e-3]])
            n = np.array([0.6, 0.8, -0.6])
            n[ax], n[(ax + 1) % 3] = v, (0.8 if m % 2 else -0.8)
            nrm.append(n)
    tri, nrm = np.array(tri), np.array(nrm)
    add(make('tolerance_normals', sm.mesh_of(tri, normals=nrm), np.ones((10, 8, 6), bool), (0.0, 0.0, 0.0), 1e-3, H6,
             max_subdiv=6, share_min=0.0))

    # ordinary inputs with defined results: a NaN vertex (n = 1, lands nowhere), a NaN area (counted; NaN is added), an
    # infinite area, an area exactly at area_epsilon (skipped), vertices at +-1e300 (span clamped), a zero normal, and an
    # area of 1e-315 whose product with a normal component of 1e-11 underflows to zero while the other two do not
    eps = 1e-320
    tri = np.array([[[2.2, 2.3, 2.4], [4.1, 2.5, 2.6], [2.7, 4.4, 3.1]],          # plain, cut 3 x 3
                    [[5.2, np.nan, 5.3], [5.4, 5.5, 5.6], [5.3, 5.7, 5.8]],      # NaN vertex
                    [[6.2, 6.3, 6.4], [6.5, 6.4, 6.6], [6.3, 6.7, 6.5]],          # NaN area
                    [[7.2, 7.3, 7.4], [7.5, 7.4, 7.6], [7.3, 7.7, 7.5]],          # infinite area
                    [[8.2, 8.3, 8.4], [8.5, 8.4, 8.6], [8.3, 8.7, 8.5]],          # area == area_epsilon
                    [[1e303, 0.0, 0.0], [-1e303, 5.0, 0.0], [0.0, 0.0, 5.0]],     # +-1e300 m
                    [[3.2, 8.3, 1.4], [3.5, 8.4, 1.6], [3.3, 8.7, 1.5]],          # zero normal
                    [[9.2, 1.3, 1.4], [9.5, 1.4, 1.6], [9.3, 1.7, 1.5]],          # underflow
                    [[6.25, 6.35, 6.45], [6.5, 6.4, 6.6], [6.3, 6.7, 6.5]]]) * 1e-3   # plain, in the NaN area's voxel
    nrm = np.array([[0.36, -0.48, 0.8], [0.6, 0.0, 0.8], [0.0, 0.6, 0.8], [-0.6, 0.0, 0.8], [0.6, 0.0, 0.8], [0.0, 0.6, 0.8],
                    [0.0, 0.0, 0.0], [1e-11, -0.6, 0.8], [0.0, -0.6, 0.8]])
    areas = np.array([2.1e-6, 4e-8, np.nan, np.inf, eps, 3e-6, 5e-8, 1e-315, 4e-8])
    cells = np.ones((12, 10, 9), bool)
    cells[7, 7, 7] = False
    add(make('special_values', sm.mesh_of(tri, normals=nrm, areas=areas), cells, (0.0, 0.0, 0.0), 1e-3,
             {'x-': 400.0, 'x+': 37.5, 'y-': -410.0, 'y+': 999.0, 'z+': 500.0}, max_subdiv=6, area_epsilon=eps,
             share_min=0.0))


if GROUP in ('margin', 'all'):
    margin_group()
if GROUP in ('boundary', 'all'):
    boundary_group()
print('reference, all cases: %d sub-triangles in %.2f s = %.1f us per sub-triangle' % (total[0], total[1],
                                                                                      1e6 * total[1] / total[0]))
