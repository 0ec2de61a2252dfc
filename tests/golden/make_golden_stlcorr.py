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

Asserted on every case, so that the reference's own binning does not hang on the last bit of a rounding: no centroid
component lies within 1e-9 dx of a voxel boundary, and no span_max at or below max_subdiv lies within 1e-9 of an integer.

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

import voxel_bc_correction as ref  # noqa: E402

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


# ---- one case -------------------------------------------------------------------------------------------------------
def dense(projected, shape):
    area = {f: np.zeros(shape) for f in FACES}
    for idx, vdata in projected.items():
        for f, a in vdata.projected_area.items():
            area[f][idx] = a
    return area


def make(name, tri, mask, origin, dx, base_h, max_subdiv=6, area_epsilon=1e-16):
    mesh = mesh_of(tri)
    origin = np.asarray(origin, dtype=float)
    nsub, dmin, smin = check_margins(mesh, origin, dx, max_subdiv, area_epsilon)
    corr = ref.STLBoundaryCorrector(mesh, mask, origin, dx, max_subdiv=max_subdiv, area_epsilon=area_epsilon)

    counts = np.zeros((6,) + mask.shape, dtype=np.uint16)
    plain_add = ref.VoxelBoundaryData.add_projected_area

    def counting_add(self, face, area):
        if area > 0.0:
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

    out = dict(triangles=mesh.triangles, normals=mesh.face_normals, areas=mesh.area_faces, mask=mask, origin=origin,
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
    print('%-12s %5d triangles %7d sub-triangles, %6d voxels hit, n_max %3d, margins %.1e dx / %.1e, '
          'reference %.2f s = %.1f us per sub-triangle, %d bytes'
          % (name, len(mesh.triangles), nsub, len(projected), counts.max(), dmin, smin, dt_plain,
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

print('reference, all cases: %d sub-triangles in %.2f s = %.1f us per sub-triangle' % (total[0], total[1],
                                                                                      1e6 * total[1] / total[0]))
