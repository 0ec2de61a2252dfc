"""Formula-built triangle meshes for the STL-correction tests and scripts/stlcorr_probe.py (no mesh library needed)."""
import math
import types

import numpy as np


def tube_triangles(centre, axis, half_len, radius, sections, rings, phase=0.0):
    """(2 * sections * rings, 3, 3) vertices: the side of a cylinder about `axis` through `centre`, `sections` x `rings`
    quads split in two, outward winding."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    a = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    th = phase + 2.0 * math.pi * np.arange(sections + 1) / sections
    circle = radius * (np.cos(th)[:, None] * e1 + np.sin(th)[:, None] * e2)                  # (sections + 1, 3)
    t = (2.0 * np.arange(rings + 1) / rings - 1.0) * half_len
    p = np.asarray(centre, dtype=np.float64) + t[:, None, None] * u + circle[None, :, :]   # (rings + 1, sections + 1, 3)
    lo0, lo1, hi0, hi1 = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    tri = np.stack([np.stack([lo0, lo1, hi1], axis=2), np.stack([lo0, hi1, hi0], axis=2)], axis=2)
    return np.ascontiguousarray(tri.reshape(-1, 3, 3))


def subdivisions(triangles, dx, max_subdiv):
    """n per triangle as voxel_bc_correction.py:70-77 takes it"""
    span = np.max((triangles.max(axis=1) - triangles.min(axis=1)) / dx, axis=1)
    n = np.where(span > 1.0, np.ceil(span), 1.0)
    return np.clip(n, 1, max_subdiv).astype(np.int64)


# ---- fixtures (tests/golden/make_golden_stlcorr.py writes them from the reference) --------------------------------------
# every centroid at least 1e-9 dx away from a voxel boundary
MARGIN_CASES = ['cyl64', 'cyl700', 'frustum', 'offgrid_sub1', 'offgrid_sub3', 'empty', 'small']
# the opposite: a stated share of the centroid components within 4 ulp of a voxel boundary (0 where the case is about
# something else), the voxel decided by the last bit of a rounding
BOUNDARY_CASES = ['box_on_planes_sub6', 'box_on_planes_sub32', 'box_f32_mm', 'box_shifted_origin', 'plate_with_holes',
                  'deep_subdiv', 'tolerance_normals', 'special_values']
HAND_SET_CASES = ['tolerance_normals', 'special_values']      # normals / areas set by hand, not from the vertices


def mesh_of(tri, normals=None, areas=None):
    """the arrays the corrector reads from a mesh object, from the vertices (cross product, its norm) or hand-set"""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).reshape(-1, 3)
        norm = np.sqrt((cross * cross).sum(axis=1))
    with np.errstate(invalid='ignore', divide='ignore'):
        unit = np.where(norm[:, None] > 0.0, cross / norm[:, None], 0.0)
    m = types.SimpleNamespace(triangles=tri, face_normals=unit if normals is None else np.asarray(normals, np.float64),
                              area_faces=norm / 2.0 if areas is None else np.asarray(areas, np.float64))
    with np.errstate(invalid='ignore', over='ignore'):
        m.triangles_center = tri.mean(axis=1) if len(tri) else np.zeros((0, 3))
    return m


def _quads(axis, plane, u0, u1, w0, w1, plus):
    """two triangles per quad at `plane` of `axis`, spanning [u0, u1] x [w0, w1] on the two following axes (cyclic);
    the winding makes the normal point along +axis when `plus`, else along -axis"""
    b, c = (axis + 1) % 3, (axis + 2) % 3
    n = len(plane)
    corner = np.zeros((4, n, 3))
    for m, (u, w) in enumerate(((u0, w0), (u1, w0), (u1, w1), (u0, w1))):
        corner[m, :, axis], corner[m, :, b], corner[m, :, c] = plane, u, w
    if not plus:
        corner = corner[::-1]
    tri = np.stack([np.stack([corner[0], corner[1], corner[2]], axis=1),
                    np.stack([corner[0], corner[2], corner[3]], axis=1)], axis=1)
    return tri.reshape(-1, 3, 3)


def box_triangles(xs, ys, zs):
    """closed surface of the axis-aligned box [xs[0], xs[-1]] x [ys[0], ys[-1]] x [zs[0], zs[-1]], every side cut into
    quads along the given coordinate lines (two values per axis: one quad per side); outward winding.  The vertices are
    the given numbers, not recomputed."""
    lines = [np.asarray(v, dtype=np.float64) for v in (xs, ys, zs)]
    out = []
    for axis in range(3):
        u, w = lines[(axis + 1) % 3], lines[(axis + 2) % 3]
        iu, iw = np.meshgrid(np.arange(len(u) - 1), np.arange(len(w) - 1), indexing='ij')
        iu, iw = iu.reshape(-1), iw.reshape(-1)
        for plus in (False, True):
            plane = np.full(len(iu), lines[axis][-1 if plus else 0])
            out.append(_quads(axis, plane, u[iu], u[iu + 1], w[iw], w[iw + 1], plus))
    return np.ascontiguousarray(np.concatenate(out))


def plate_triangles(mask, planes):
    """the surface of a voxel set as axis-aligned unit quads (two triangles each, outward winding): one quad per face
    between an in-mask voxel and an off-mask one or the outside.  planes[a][i] is the coordinate of the voxel boundary i
    along axis a (len = extent + 1).  A plate with through-holes is one such set."""
    mask = np.asarray(mask, dtype=bool)
    out = []
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        m = np.moveaxis(mask, axis, 0)
        for plus in (False, True):
            nb = np.zeros_like(m)
            if plus:
                nb[:-1] = m[1:]
            else:
                nb[1:] = m[:-1]
            idx = np.stack(np.nonzero(np.moveaxis(m & ~nb, 0, axis)), axis=1)
            pa, pb, pc = (np.asarray(planes[a], dtype=np.float64) for a in (axis, b, c))
            out.append(_quads(axis, pa[idx[:, axis] + (1 if plus else 0)], pb[idx[:, b]], pb[idx[:, b] + 1],
                              pc[idx[:, c]], pc[idx[:, c] + 1], plus))
    return np.ascontiguousarray(np.concatenate(out))


def soup_triangles(rng, count, lo, hi, extent, lattice):
    """`count` random triangles: a corner uniform in the box [lo, hi] and two more within `extent` of it, every vertex
    snapped to whole multiples of `lattice` (snapping is what puts centroids on voxel boundaries)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    first = rng.uniform(lo, hi, (count, 1, 3))
    size = rng.uniform(0.05, 1.0, (count, 1, 1)) * extent
    tri = np.concatenate([first, first + rng.uniform(-1.0, 1.0, (count, 2, 3)) * size], axis=1)
    return np.round(tri / lattice) * lattice


# ---- the seeded fuzz of test_stlcorr_gpu.py ---------------------------------------------------------------------------
FUZZ_SEEDS = 40
FUZZ_BUDGET = 60000                      # sub-triangles per case: a few seconds of the oracle for the whole fuzz
_EXTENTS = (1, 2, 7, 16, 17, 33, 40, 100)
_RAGGED = ((37, 29, 50), (45, 23, 61))   # the device layout pads these
_SUBDIV = (1, 2, 5, 6, 7, 16, 33, 64)
_MESHES = ('box', 'plate', 'soup', 'tube', 'tube_axis')
_MASKS = ('all', 'solid', 'holes', 'walls')
_DX = (2.5e-4, 1e-3, 2.0 ** -10)
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')


def _fuzz_mask(kind, shape, rng):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'), axis=-1)
    if kind == 'all':
        return np.ones(shape, bool)
    if kind == 'solid':                                         # an ellipsoid that touches the box
        half = np.array(shape) / 2.0
        return (((idx + 0.5 - half) / half) ** 2).sum(axis=-1) <= 1.0
    if kind == 'holes':
        return rng.random(shape) >= 0.3
    p = rng.integers(3, 6, 3)                                   # walls one voxel thick
    return (idx[..., 0] % p[0] == 0) | (idx[..., 1] % p[1] == 0) | (idx[..., 2] % p[2] == p[2] - 1)


def fuzz_case(seed):
    """-> namespace(mesh, mask, origin, dx, max_subdiv, area_epsilon, base_h, mesh_kind, mask_kind); the same case for
    the same seed, wherever it is built"""
    rng = np.random.default_rng(20260 + seed)
    max_subdiv = _SUBDIV[seed % 8]
    mesh_kind = _MESHES[(seed // 8 + seed) % 5]
    mask_kind = _MASKS[(seed // 3) % 4]
    dx = _DX[(seed // 2) % 3]
    if seed % 10 == 9:
        shape = _RAGGED[(seed // 10) % 2]
    else:
        shape = tuple(int(rng.choice(_EXTENTS)) for _ in range(3))
        if max_subdiv >= 16 and max(shape) < 16:               # room for a deep cut
            shape = (shape[0], 40, shape[2])
    mask = _fuzz_mask(mask_kind, shape, rng)
    if not mask.any():
        mask[...] = True
    # the origin: whole voxels on odd seeds (lattice vertices then give centroids ON boundaries), anything on even ones
    origin = rng.integers(-3, 4, 3) * dx if seed % 2 else rng.uniform(-3.0, 3.0, 3) * dx
    ext = np.array(shape, dtype=np.float64)
    if mesh_kind == 'box':
        lo = np.array([int(rng.integers(-1, max(1, n // 3))) for n in shape])
        hi = np.array([int(rng.integers(l + 1, n + 2)) for l, n in zip(lo, shape)])
        cuts = [int(rng.integers(1, 4)) for _ in range(3)]
        lines = [origin[a] + np.unique(np.round(np.linspace(lo[a], hi[a], cuts[a] + 1))) * dx for a in range(3)]
        tri = box_triangles(*lines)
    elif mesh_kind == 'plate':
        tri = plate_triangles(mask, [origin[a] + np.arange(shape[a] + 1) * dx for a in range(3)])
    elif mesh_kind == 'soup':
        lattice = dx / (2.0, 3.0, 8.0)[seed % 3]
        size = rng.uniform(2.0, 1.4 * max(max_subdiv, 3)) * dx
        tri = origin + soup_triangles(rng, 4000, -2.0 * dx, (ext + 2.0) * dx, size, lattice)
    else:
        axis = (0.3, 0.2, 1.0) if mesh_kind == 'tube' else ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))[seed % 3]
        radius = 0.45 * float(np.sort(ext)[1]) * dx
        sections = int(rng.integers(5, 40))
        tri = tube_triangles(origin + 0.5 * ext * dx, axis, 0.4 * float(ext.max()) * dx, radius, sections,
                             int(rng.integers(1, 6)), phase=float(rng.uniform(0.0, 1.0)))
    # keep the case within the budget: drop triangles at random, the order of the rest stays
    cost = subdivisions(tri, dx, max_subdiv) ** 2
    if cost.sum() > FUZZ_BUDGET:
        order = rng.permutation(len(tri))
        keep = np.sort(order[np.cumsum(cost[order]) <= FUZZ_BUDGET])
        tri = tri[keep]
    mesh = mesh_of(tri)
    area_epsilon = 1e-16 if seed % 4 else float(np.median(mesh.area_faces))
    faces = [f for f in FACES if rng.random() < 0.7] or ['z+']
    base_h = {f: float(np.round(rng.uniform(5.0, 900.0), 2)) for f in rng.permutation(faces)}
    base_h[faces[0]] = 0.0
    if len(faces) > 2:
        base_h[faces[1]] = -base_h[faces[1]]
    return types.SimpleNamespace(mesh=mesh, mask=mask, origin=origin, dx=dx, max_subdiv=max_subdiv,
                                 area_epsilon=area_epsilon, base_h=base_h, mesh_kind=mesh_kind, mask_kind=mask_kind)
