"""The CPU statement of the solid voxelisation: NumPy fp64, plus the same rule in exact rational
arithmetic for small cases, plus the closed meshes and closed-form inside tests the voxeliser tests share.

Definition.  Ray axis a, b = (a + 1) % 3, c = (a + 2) % 3; the centre of voxel i along axis m is
origin[m] + (i + 0.5) * dx.
  cover   a triangle covers column (u, w) when the three edge functions of its projection onto (b, c) have one strict
          sign; each edge is evaluated with its endpoints in lexicographic (u, w) order and the sign flipped back; a
          zero takes the sign of the column nudged by (+eps, +eps^2): -sign(dw) if the ordered edge has dw != 0, else
          sign(du).  Zero projected area covers nothing.
  depth   d0 + (l1 * (d1 - d0) + l2 * (d2 - d0)), l1 and l2 the barycentric weights from the projected coordinates.
  toggle  the crossing toggles every voxel of the column whose centre is >= depth.
  solid   odd number of toggles; a column whose total is odd is a leak.
"""
import math
from fractions import Fraction

import numpy as np

from stlcorr_meshes import tube_triangles


def _side(au, aw, bu, bw, pu, pw):
    swap = (au > bu) | ((au == bu) & (aw > bw))
    au, bu = np.where(swap, bu, au), np.where(swap, au, bu)
    aw, bw = np.where(swap, bw, aw), np.where(swap, aw, bw)
    du, dw = bu - au, bw - aw
    e = du * (pw - aw) - dw * (pu - au)
    s = np.sign(e)
    tie = np.where(dw != 0, -np.sign(dw), np.sign(du))
    s = np.where(s == 0, tie, s)
    return np.where(swap, -s, s)


def _range(lo, hi, o, dx, n, clip):
    """columns whose centre may lie in [lo, hi], one column of margin on either side; all of them without `clip`"""
    if not clip:
        return 0, n - 1
    a, b = math.floor((lo - o) / dx - 0.5) - 1.0, math.ceil((hi - o) / dx - 0.5) + 1.0
    if not a <= b or not b >= 0.0 or not a <= n - 1:
        return 0, -1
    return int(max(a, 0.0)), int(min(b, n - 1.0))


def voxelize(tri, origin, dx, shape, axis, clip=True):
    """-> (solid (nx, ny, nz) bool, leaking columns).  `clip` tests only the columns of a triangle's bounding box, which
    is what makes large cases affordable; clip=False tests every column against every triangle."""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    origin = np.asarray(origin, dtype=np.float64)
    dx = float(dx)
    b, c = (axis + 1) % 3, (axis + 2) % 3
    nd, nu, nw = shape[axis], shape[b], shape[c]
    cu = origin[b] + (np.arange(nu) + 0.5) * dx
    cw = origin[c] + (np.arange(nw) + 0.5) * dx
    cd = origin[axis] + (np.arange(nd) + 0.5) * dx
    tog = np.zeros((nd + 1, nu, nw), dtype=np.int64)
    with np.errstate(all='ignore'):
        for t in tri:
            d0, d1, d2 = t[:, axis]
            u0, u1, u2 = t[:, b]
            w0, w1, w2 = t[:, c]
            A = (u1 - u0) * (w2 - w0) - (w1 - w0) * (u2 - u0)
            if A == 0 or A != A:
                continue
            fu, lu = _range(np.fmin.reduce(t[:, b]), np.fmax.reduce(t[:, b]), origin[b], dx, nu, clip)
            fw, lw = _range(np.fmin.reduce(t[:, c]), np.fmax.reduce(t[:, c]), origin[c], dx, nw, clip)
            if lu < fu or lw < fw:
                continue
            PU, PW = np.meshgrid(cu[fu:lu + 1], cw[fw:lw + 1], indexing='ij')
            s0, s1, s2 = _side(u0, w0, u1, w1, PU, PW), _side(u1, w1, u2, w2, PU, PW), _side(u2, w2, u0, w0, PU, PW)
            cov = ((s0 > 0) & (s1 > 0) & (s2 > 0)) | ((s0 < 0) & (s1 < 0) & (s2 < 0))
            if not cov.any():
                continue
            l1 = ((PU - u0) * (w2 - w0) - (PW - w0) * (u2 - u0)) / A
            l2 = ((u1 - u0) * (PW - w0) - (w1 - w0) * (PU - u0)) / A
            depth = d0 + (l1 * (d1 - d0) + l2 * (d2 - d0))
            idx = np.searchsorted(cd, depth[cov], side='left')       # the first voxel whose centre is >= depth; NaN: none
            ju, jw = np.nonzero(cov)
            np.add.at(tog, (idx, ju + fu, jw + fw), 1)
    par = np.cumsum(tog, axis=0) % 2
    solid = np.moveaxis(par[:-1].astype(bool), [0, 1, 2], [axis, b, c])
    return np.ascontiguousarray(solid), int(par[-1].sum())


def voxelize_majority(tri, origin, dx, shape):
    res = [voxelize(tri, origin, dx, shape, a) for a in range(3)]
    votes = sum(m.astype(np.int8) for m, _ in res)
    return votes >= 2, tuple(l for _, l in res)


# ---- the same rule in exact rational arithmetic --------------------------------------------------------------------
def _sgn(x):
    return (x > 0) - (x < 0)


def _side_exact(a, b, p):
    swap = a > b                               # tuples compare lexicographically
    if swap:
        a, b = b, a
    du, dw = b[0] - a[0], b[1] - a[1]
    s = _sgn(du * (p[1] - a[1]) - dw * (p[0] - a[0]))
    if s == 0:
        s = -_sgn(dw) if dw != 0 else _sgn(du)
    return -s if swap else s


def voxelize_exact(tri, origin, dx, shape, axis):
    """`voxelize` with every number a Fraction: what the definition means where the doubles round.  Small cases only."""
    F = Fraction
    tri = [[[F(float(x)) for x in v] for v in t] for t in np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)]
    origin = [F(float(o)) for o in origin]
    dx = F(float(dx))
    b, c = (axis + 1) % 3, (axis + 2) % 3
    nd, nu, nw = shape[axis], shape[b], shape[c]
    half = F(1, 2)
    cu = [origin[b] + (i + half) * dx for i in range(nu)]
    cw = [origin[c] + (i + half) * dx for i in range(nw)]
    cd = [origin[axis] + (i + half) * dx for i in range(nd)]
    tog = np.zeros((nd + 1, nu, nw), dtype=np.int64)
    for t in tri:
        d = [v[axis] for v in t]
        q = [(v[b], v[c]) for v in t]
        A = (q[1][0] - q[0][0]) * (q[2][1] - q[0][1]) - (q[1][1] - q[0][1]) * (q[2][0] - q[0][0])
        if A == 0:
            continue
        ulo, uhi = min(v[0] for v in q), max(v[0] for v in q)
        wlo, whi = min(v[1] for v in q), max(v[1] for v in q)
        for iu in range(nu):
            if not ulo <= cu[iu] <= uhi:       # exact: a centre outside the closed bounding box is not covered
                continue
            for iw in range(nw):
                if not wlo <= cw[iw] <= whi:
                    continue
                p = (cu[iu], cw[iw])
                s = [_side_exact(q[m], q[(m + 1) % 3], p) for m in range(3)]
                if not (all(x > 0 for x in s) or all(x < 0 for x in s)):
                    continue
                l1 = ((p[0] - q[0][0]) * (q[2][1] - q[0][1]) - (p[1] - q[0][1]) * (q[2][0] - q[0][0])) / A
                l2 = ((q[1][0] - q[0][0]) * (p[1] - q[0][1]) - (q[1][1] - q[0][1]) * (p[0] - q[0][0])) / A
                depth = d[0] + (l1 * (d[1] - d[0]) + l2 * (d[2] - d[0]))
                idx = next((i for i in range(nd) if cd[i] >= depth), nd)
                tog[idx, iu, iw] += 1
    par = np.cumsum(tog, axis=0) % 2
    solid = np.moveaxis(par[:-1].astype(bool), [0, 1, 2], [axis, b, c])
    return np.ascontiguousarray(solid), int(par[-1].sum())


# ---- closed meshes with a closed-form inside test --------------------------------------------------------------------
def closed_tube(centre, axis, half, radius, sections, rings):
    """the side of tube_triangles closed with two fan caps -> (triangles, unit axis)"""
    side = tube_triangles(centre, axis, half, radius, sections, rings)
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    quads = side.reshape(rings, sections, 2, 3, 3)
    ring_lo = quads[0, :, 0, :2]                    # lo0, lo1 of the first ring
    ring_hi = quads[-1, :, 1, 1:][:, ::-1]          # hi0, hi1 of the last
    clo, chi = np.asarray(centre, dtype=np.float64) - half * u, np.asarray(centre, dtype=np.float64) + half * u
    caps = []
    for s in range(sections):
        caps.append([clo, ring_lo[s, 1], ring_lo[s, 0]])
        caps.append([chi, ring_hi[s, 0], ring_hi[s, 1]])
    return np.ascontiguousarray(np.concatenate([side, np.array(caps)])), u


def centres(origin, dx, shape):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'), axis=-1)
    return np.asarray(origin, dtype=np.float64) + (idx + 0.5) * dx


def prism_distance(origin, dx, shape, centre, axis, half, radius, sections, phase=0.0):
    """signed distance-like function of the regular `sections`-gon prism of closed_tube: negative inside, its modulus a
    lower bound of the distance to the surface near it (the largest of the half-space functions)"""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    a = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    P = centres(origin, dx, shape) - np.asarray(centre, dtype=np.float64)
    x, y, along = P @ e1, P @ e2, P @ u
    th = phase + 2.0 * math.pi * np.arange(sections) / sections + math.pi / sections
    apothem = radius * math.cos(math.pi / sections)
    dist = np.full(P.shape[:-1], -np.inf)
    for t in th:                                    # one half plane at a time: no (cells, sections) temporary
        np.maximum(dist, x * math.cos(t) + y * math.sin(t) - apothem, out=dist)
    return np.maximum(dist, np.abs(along) - half)


def octahedron_triangles(centre, radii):
    """the octahedron |x - cx| / rx + |y - cy| / ry + |z - cz| / rz <= 1: eight slanted faces, outward winding"""
    c = np.asarray(centre, dtype=np.float64)
    r = np.asarray(radii, dtype=np.float64)
    out = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                v = [c + np.array([sx * r[0], 0, 0]), c + np.array([0, sy * r[1], 0]), c + np.array([0, 0, sz * r[2]])]
                if sx * sy * sz < 0:
                    v = v[::-1]
                out.append(v)
    return np.array(out)


def octahedron_distance(origin, dx, shape, centre, radii):
    """(|x| / rx + |y| / ry + |z| / rz - 1) scaled to a length: negative inside, modulus a lower bound of the distance to
    the surface (the gradient of the unscaled function is at most sqrt(3) / min(r))"""
    P = np.abs(centres(origin, dx, shape) - np.asarray(centre, dtype=np.float64))
    r = np.asarray(radii, dtype=np.float64)
    return ((P / r).sum(axis=-1) - 1.0) * (float(r.min()) / math.sqrt(3.0))


def geodesic_polyhedron(centre, radius, level):
    """an icosahedron subdivided `level` times with the new vertices pushed onto the sphere: a closed convex polyhedron
    -> (triangles, unit outward face normals, face offsets) with inside == all(n . (p - centre) < offset)"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], dtype=np.float64)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v /= np.linalg.norm(v[0])
    tri = v[np.array(f)]
    for _ in range(level):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = (a + b), (b + c), (c + a)
        ab, bc, ca = (m / np.linalg.norm(m, axis=1, keepdims=True) for m in (ab, bc, ca))
        tri = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1),
                              np.stack([ab, bc, ca], 1)])
    # a vertex shared by several triangles must be the same double in all of them: a + b and b + a are
    tri = np.asarray(centre, dtype=np.float64) + radius * tri
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    off = np.einsum('ij,ij->i', n, tri[:, 0] - np.asarray(centre, dtype=np.float64))
    return np.ascontiguousarray(tri), n, off


def polyhedron_distance(origin, dx, shape, centre, normals, offsets):
    """max over the faces of n . (p - centre) - offset: negative inside a convex polyhedron, modulus a lower bound of the
    distance to its surface near it"""
    P = centres(origin, dx, shape) - np.asarray(centre, dtype=np.float64)
    dist = np.full(P.shape[:-1], -np.inf)
    for n, o in zip(normals, offsets):
        np.maximum(dist, P @ n - o, out=dist)
    return dist


def write_binary_stl(path, tri):
    """binary STL from (n, 3, 3) vertices with the standard library; normals left zero, as many writers do"""
    import struct
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    with open(path, 'wb') as f:
        f.write(b'voxelize test'.ljust(80, b' '))
        f.write(struct.pack('<I', len(tri)))
        for t in tri:
            f.write(struct.pack('<12fH', 0.0, 0.0, 0.0, *[float(x) for x in t.reshape(-1)], 0))


# ---- cases the CPU and the GPU tests share -----------------------------------------------------------------------------
DYADIC_DX = 2.0 ** -10


def dyadic_cases():
    """[(name, triangles, origin, dx, shape)]: closed meshes whose vertices and grid origin are whole multiples of dx / 8
    with dx = 2^-10 and extents <= 16, the octahedra with power-of-two radii: every product, sum and quotient of the
    definition is then exact in doubles, and the fp64 statement must equal the rational one"""
    from stlcorr_meshes import box_triangles, plate_triangles
    dx = DYADIC_DX
    rng = np.random.default_rng(11)
    out = []
    for n, shape in enumerate(((9, 7, 11), (5, 16, 6))):
        mask = rng.random(shape) >= 0.35
        org = np.array([3, -2, 5]) * dx + rng.integers(-8, 9, 3) * (dx / 8)
        planes = [org[a] + np.arange(shape[a] + 1) * dx for a in range(3)]
        tri = plate_triangles(mask, planes)
        out.append(('plate%d_general' % n, tri, org, dx, shape))
        # centres ON the mesh planes, edges and vertices
        out.append(('plate%d_on_planes' % n, tri, org - dx / 2, dx, tuple(s + 1 for s in shape)))
        # planes an eighth of a voxel off the centres
        out.append(('plate%d_eighth' % n, tri, org - 3 * dx / 8, dx, tuple(s + 1 for s in shape)))
    org = np.array([-4, 7, 1]) * dx
    lines = [org[a] + np.array([1, 3, 4, 6]) * dx for a in range(3)]
    out.append(('cut_box_on_vertices', box_triangles(*lines), org - dx / 2, dx, (8, 8, 8)))
    lines = [org[a] + np.array([9, 21, 30, 51]) * (dx / 8) for a in range(3)]
    out.append(('cut_box_eighths', box_triangles(*lines), org, dx, (8, 7, 9)))
    for name, off in (('octa_on_centres', 0.5), ('octa_on_planes', 0.0), ('octa_eighth', 0.375)):
        c = org + (np.array([6, 5, 8]) + off) * dx
        out.append((name, octahedron_triangles(c, np.array([4.0, 2.0, 8.0]) * dx), org, dx, (13, 10, 16)))
    return out


VOX_FUZZ_SEEDS = 24
_VOX_SHAPES = ((1, 1, 1), (2, 7, 3), (16, 17, 5), (33, 8, 40), (37, 29, 50), (12, 40, 70), (7, 33, 16), (40, 16, 33))
_VOX_DX = (2.5e-4, 1e-3, 2.0 ** -10)
_VOX_MESHES = ('plate', 'box', 'prism', 'octa', 'geodesic')


def fuzz_case(seed):
    """-> (kind, triangles, origin, dx, shape, axis): a closed mesh, a grid it may stick out of, a ray axis; the same
    case for the same seed wherever it is built"""
    from stlcorr_meshes import _fuzz_mask, box_triangles, plate_triangles
    rng = np.random.default_rng(77100 + seed)
    kind = _VOX_MESHES[seed % 5]
    dx = _VOX_DX[(seed // 2) % 3]
    shape = _VOX_SHAPES[(seed // 3 + seed) % 8]
    axis = (seed // 5 + 2 * (seed % 5)) % 3
    # whole voxels or half voxels on odd seeds (vertices of lattice meshes on centres and planes), anything on even ones
    origin = rng.integers(-6, 7, 3) * (dx / 2) if seed % 2 else rng.uniform(-3.0, 3.0, 3) * dx
    ext = np.array(shape, dtype=np.float64)
    if kind == 'plate':
        mask = _fuzz_mask(('holes', 'walls', 'solid')[(seed // 5) % 3], shape, rng)
        shift = (0.0, 0.5)[(seed // 15) % 2] * dx
        tri = plate_triangles(mask, [origin[a] + shift + np.arange(shape[a] + 1) * dx for a in range(3)])
    elif kind == 'box':
        lo = np.array([int(rng.integers(-2, max(1, n // 3))) for n in shape])
        hi = np.array([int(rng.integers(l + 1, n + 3)) for l, n in zip(lo, shape)])
        lines = [origin[a] + np.unique(np.round(np.linspace(lo[a], hi[a], int(rng.integers(1, 4)) + 1) * 2) / 2) * dx
                 for a in range(3)]
        tri = box_triangles(*lines)
    elif kind == 'prism':
        tri, _ = closed_tube(origin + 0.5 * ext * dx, rng.uniform(-1.0, 1.0, 3) + np.array([0.0, 0.0, 1.5]),
                             0.45 * float(ext.max()) * dx, 0.4 * float(np.sort(ext)[1]) * dx, int(rng.integers(3, 40)),
                             int(rng.integers(1, 5)))
    elif kind == 'octa':
        tri = octahedron_triangles(origin + np.round(ext * rng.uniform(0.3, 0.7, 3) * 2) / 2 * dx,
                                   np.maximum(1.0, np.round(ext * rng.uniform(0.2, 0.7, 3))) * dx)
    else:
        tri, _, _ = geodesic_polyhedron(origin + 0.5 * ext * dx, 0.45 * float(ext.max()) * dx, int(rng.integers(0, 3)))
    return kind, np.ascontiguousarray(tri), origin, dx, shape, axis
