"""GPU: the STL correction of voxel Robin coefficients (adi_thermal_fields_amd.voxel_bc_correction, csrc/adi_stlcorr.hip)
against the reference's fields (tests/golden/stlcorr_*.npz, written by tests/golden/make_golden_stlcorr.py).

Bounds.  The set of non-zero cells of every field must be the reference's exactly: that is the binning.  Seven fixtures
keep every centroid at least 1e-9 dx away from a voxel boundary; eight more do the opposite (planar faces on voxel planes,
whole-voxel spans, normals at the 1e-12 tolerance, NaN / huge / subnormal inputs: stlcorr_meshes.BOUNDARY_CASES), so the
voxel of a sub-triangle hangs on the last bit of a rounding and the device has to round as NumPy does.  Beyond the
fixtures the reference is oracle/stlcorr_oracle.py, pinned to them bit for bit on the CPU
(test_oracle_stlcorr_golden.py): a seeded fuzz over meshes, shapes, masks and depths, the slot decode down to
max_subdiv = 4096 on the C ABI, special values.  A value may differ by n_max * 2^-52 relative, the bound
for sums of n_max positive terms taken in another order, n_max read from the fixture; the device adds in the
reference's order, so the differences measured so far are zero.  At scale there is no reference: for an
all-true mask that contains the mesh every sub-triangle lands, so each projected-area field sums to
sum(area * max(+-n_c, 0)) over the triangles, within N * 2^-52 relative for N sub-triangles.
"""
import math
import os

import numpy as np
import pytest

import cases
from helpers import GOLDEN, rel_linf
import stlcorr_meshes as sm
from stlcorr_meshes import subdivisions, tube_triangles

pytestmark = pytest.mark.gpu

FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
CASES = sm.MARGIN_CASES + sm.BOUNDARY_CASES
EPS = 2.0 ** -52


class Mesh:
    """the fixture's arrays as the mesh object the reference was given"""

    def __init__(self, g):
        self.triangles, self.face_normals, self.area_faces = g['triangles'], g['normals'], g['areas']
        self.triangles_center = g['triangles'].mean(axis=1)


def _load(name):
    g = np.load(os.path.join(GOLDEN, 'stlcorr_%s.npz' % name))
    base_h = {str(f): float(v) for f, v in zip(g['base_faces'], g['base_vals'])}
    return g, base_h


def _corrector(g, mask=None):
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector
    return STLBoundaryCorrector(Mesh(g), g['mask'] if mask is None else mask, g['origin'], float(g['dx']),
                                max_subdiv=int(g['max_subdiv']), area_epsilon=float(g['area_epsilon']))


def _compare(what, got, want, n_max):
    """same non-zero cells, values within n_max * 2^-52 relative; -> largest relative difference"""
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(got != 0.0, want != 0.0), '%s: %d cells differ in being zero' % (
        what, int(np.count_nonzero((got != 0.0) != (want != 0.0))))
    odd = ~np.isfinite(want)                       # a NaN or an infinite area in the mesh: the same NaN / infinity
    assert np.array_equal(got[odd], want[odd], equal_nan=True), what
    nz = (want != 0.0) & ~odd
    worst = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0
    assert worst <= n_max * EPS, '%s: relative difference %.3e above %d * 2^-52' % (what, worst, n_max)
    return worst


@pytest.mark.parametrize('fallback', [True, False], ids=['fallback', 'nofallback'])
@pytest.mark.parametrize('name', CASES)
def test_fields_equal_the_reference(name, fallback):
    g, base_h = _load(name)
    n_max, tag = int(g['n_max']), 'on' if fallback else 'off'
    robin, scale = _corrector(g).build_corrected_fields(base_h, fallback_to_base=fallback)
    assert list(robin) == list(base_h) and list(scale) == list(base_h)          # the reference's keys, in its order
    worst = 0.0
    for f in base_h:
        worst = max(worst, _compare('robin ' + f, robin[f], g['robin_%s_%s' % (tag, f)], n_max),
                    _compare('scale ' + f, scale[f], g['scale_%s_%s' % (tag, f)], n_max))
        if fallback and base_h[f] != 0.0:
            fell = (g['count'][FACES.index(f)] == 0) & (g['robin_on_' + f] != 0.0)   # no contribution, yet a value
            assert np.all(robin[f][fell] == base_h[f]) and np.all(scale[f][fell] == 1.0), f
        if base_h[f] == 0.0:
            assert not robin[f].any() and not scale[f].any(), f
    print('STLCORR %s %s: %d sub-triangles, n_max %d, largest relative difference %.3e (bound %.3e)'
          % (name, tag, int(g['n_sub']), n_max, worst, n_max * EPS))


@pytest.mark.parametrize('name', CASES)
def test_projected_area_fields_equal_the_reference(name):
    g, _ = _load(name)
    area = _corrector(g).projected_area_fields()
    assert list(area) == list(FACES)
    worst = max(_compare('area ' + f, area[f], g['area_' + f], int(g['n_max'])) for f in FACES)
    assert all(np.array_equal(area[f] != 0.0, g['count'][i] != 0) for i, f in enumerate(FACES))
    print('STLCORR area %s: largest relative difference %.3e' % (name, worst))


def test_wrapper_and_device_mask_give_the_same_fields():
    """build_corrected_robin_fields (the reference's helper) on a NumPy mask, and the corrector on a device mask: tensor,
    bool tensor and DeviceField"""
    import torch
    from adi_thermal_fields_amd.adi3d_hip_coeff import DeviceField
    from adi_thermal_fields_amd.voxel_bc_correction import build_corrected_robin_fields
    g, base_h = _load('cyl64')
    robin, scale = build_corrected_robin_fields(Mesh(g), g['mask'], g['origin'], float(g['dx']), base_h)
    for f in base_h:
        _compare('robin ' + f, robin[f], g['robin_on_' + f], int(g['n_max']))
        _compare('scale ' + f, scale[f], g['scale_on_' + f], int(g['n_max']))
    d_bool = torch.from_numpy(g['mask']).cuda()
    for m in (d_bool, d_bool.to(torch.uint8), DeviceField(d_bool.to(torch.float64))):
        r2, s2 = _corrector(g, mask=m).build_corrected_fields(base_h)
        for f in base_h:
            assert isinstance(r2[f], torch.Tensor) and r2[f].is_cuda and r2[f].dtype == torch.float64
            assert np.array_equal(r2[f].cpu().numpy(), robin[f]) and np.array_equal(s2[f].cpu().numpy(), scale[f]), f


def test_two_runs_give_the_same_bits():
    import torch
    g, base_h = _load('cyl700')
    d_mask = torch.from_numpy(g['mask']).cuda()
    a = _corrector(g, mask=d_mask).build_corrected_fields(base_h)
    b = _corrector(g, mask=d_mask).build_corrected_fields(base_h)
    for x, y in zip(a, b):
        for f in base_h:
            assert torch.equal(x[f], y[f]), f
    pa, pb = _corrector(g, mask=d_mask).projected_area_fields(), _corrector(g, mask=d_mask).projected_area_fields()
    assert all(torch.equal(pa[f], pb[f]) for f in FACES)


@pytest.mark.parametrize('name', ['cyl64', 'frustum'])
def test_packs_from_device_fields_step_like_the_oracle(name):
    """mask and fields never leave HBM: Grid3D's device mask -> corrector -> robin_h of precompute_coeff_packs_unified ->
    three Cartesian steps, against the pinned oracle fed with the reference's (golden) fields"""
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    g, base_h = _load(name)
    shape, dx, mask = g['mask'].shape, float(g['dx']), g['mask']
    mat = dict(cases.STEEL)
    rng = np.random.default_rng(11)
    T0 = np.where(mask, rng.uniform(20.0, 1000.0, shape), 20.0)
    dt = 40.0 * dx * dx / (mat['k'] / (mat['rho'] * mat['cp']))

    grid = hip.Grid3D(*shape, dx, mask)
    robin, _ = _corrector(g, mask=grid.d_mask).build_corrected_fields(base_h)
    for f in base_h:
        assert grid.layout.is_native(robin[f]), f                                 # taken as it is: no copy, no host trip
    packs = hip.precompute_coeff_packs_unified(grid, hip.Material(**mat), robin_h=robin)
    T = hip.to_device(T0)
    for _ in range(3):
        T = hip.adi_step_hip_coeff(T, grid, hip.Material(**mat), hip.Params(dt, 0.5), packs, Tinf=20.0)
    got = np.asarray(T)

    ogrid = orc.Grid3D(*shape, dx, mask)
    opacks = orc.precompute_coeff_packs_unified(ogrid, orc.Material(**mat),
                                                robin_h={f: g['robin_on_' + f] for f in base_h})
    for a in range(3):
        assert rel_linf(np.asarray(packs[a].coeff), opacks[a].coeff) <= 1e-10, a
    Tw = T0
    for _ in range(3):
        Tw = orc.adi_step_numba_coeff(Tw, ogrid, orc.Material(**mat), orc.Params(dt, 0.5), opacks, Tinf=20.0)
    e = rel_linf(got, Tw)
    print('STLCORR end to end %s: rel_linf %.3e after three steps' % (name, e))
    assert e <= 1e-10, e
    assert np.abs(Tw - T0).max() > 1.0                                           # the steps did something


def _expected_sums(mesh):
    """per face: fsum(area * max(+-n_c, 0)) over triangles with |n_c| > 1e-12"""
    out = {}
    for ax in range(3):
        c = mesh.face_normals[:, ax]
        out[FACES[2 * ax + 1]] = math.fsum((mesh.area_faces * c)[c > 1e-12].tolist())
        out[FACES[2 * ax]] = math.fsum((mesh.area_faces * -c)[c < -1e-12].tolist())
    return out


def _fsum_field(t):
    """exact sum of a device field's non-zero cells (there are few), and the flat index of the first of them"""
    import torch
    flat = t.reshape(-1) if t.is_contiguous() else t.contiguous().reshape(-1)
    idx = torch.nonzero(flat).reshape(-1)
    return math.fsum(flat[idx].cpu().tolist()), idx


def test_a_million_triangles_in_512_cubed():
    """no reference at this size (tens of minutes of CPython): conservation of the projected area, and two runs alike"""
    import torch
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector, TriangleMesh
    dx, n = 1e-3, 512
    mesh = TriangleMesh(tube_triangles((0.256, 0.256, 0.256), (0.3, 0.2, 1.0), 0.2, 0.18, 1000, 500, phase=0.01))
    assert len(mesh) == 1000000 and mesh.triangles.min() > dx and mesh.triangles.max() < (n - 1) * dx
    N = int((subdivisions(mesh.triangles, dx, 6) ** 2).sum())
    mask = torch.ones((n, n, n), dtype=torch.uint8, device='cuda')
    corr = STLBoundaryCorrector(mesh, mask, (0.0, 0.0, 0.0), dx)
    want = _expected_sums(mesh)
    area = corr.projected_area_fields()
    worst = 0.0
    for f in FACES:
        got, _ = _fsum_field(area[f])
        rel = abs(got - want[f]) / want[f]
        worst = max(worst, rel)
        assert rel <= N * EPS, (f, got, want[f], rel, N * EPS)
    print('STLCORR scale: %d triangles, %d sub-triangles, largest relative difference of a face sum %.3e (bound %.3e)'
          % (len(mesh), N, worst, N * EPS))
    again = corr.projected_area_fields()
    assert all(torch.equal(area[f], again[f]) for f in FACES)


@pytest.mark.parametrize('shape', [(1100, 512, 512), (2100, 1024, 1024)], ids=['past_2GiB', 'past_2^31_cells'])
def test_keys_past_32_bits(shape):
    """a mesh in the far corner of a grid whose fp64 fields pass 2 GiB, and of one with more than 2^31 cells: keys, cell
    offsets and the fallback's thread numbers are 64-bit"""
    import torch
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector, TriangleMesh
    dx = 1e-3
    far = np.array(shape, dtype=np.float64) * dx
    mesh = TriangleMesh(tube_triangles(far - 0.02, (0.3, 0.2, 1.0), 0.012, 0.011, 240, 60, phase=0.01))
    assert np.all(mesh.triangles.min(axis=(0, 1)) > far - 0.04) and np.all(mesh.triangles.max(axis=(0, 1)) < far - dx)
    N = int((subdivisions(mesh.triangles, dx, 6) ** 2).sum())
    mask = torch.ones(shape, dtype=torch.uint8, device='cuda')
    base = 250.0
    robin, scale = STLBoundaryCorrector(mesh, mask, (0.0, 0.0, 0.0), dx).build_corrected_fields({'x+': base})
    del mask
    want = _expected_sums(mesh)['x+'] / (dx * dx)
    # with the fallback the last plane (exposed on x+, never reached by the mesh) holds scale 1 and nothing else does
    assert torch.all(scale['x+'][-1] == 1.0) and torch.all(robin['x+'][-1] == base)
    body = scale['x+'][:-1]
    assert body.stride(0) * (shape[0] - 40) * 8 > 1 << 31
    got, idx = _fsum_field(body[shape[0] - 41:])
    assert not body[:shape[0] - 41].any()
    first = int(idx[0]) + (shape[0] - 41) * shape[1] * shape[2]
    assert first * 8 > 1 << 31 and (shape[0] < 2100 or first > 1 << 31), first
    rel = abs(got - want) / want
    print('STLCORR far corner %s: first cell %d, relative difference of the scale sum %.3e (bound %.3e)'
          % (shape, first, rel, N * EPS))
    assert rel <= N * EPS, (got, want, rel)


# ---- against the oracle -----------------------------------------------------------------------------------------------
def _oracle(c):
    from oracle import stlcorr_oracle as orc
    return orc.STLBoundaryCorrector(c.mesh, c.mask, c.origin, c.dx, max_subdiv=c.max_subdiv, area_epsilon=c.area_epsilon)


def _device(c, mask):
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector
    return STLBoundaryCorrector(c.mesh, mask, c.origin, c.dx, max_subdiv=c.max_subdiv, area_epsilon=c.area_epsilon)


def _whole_storage(t):
    """every element of the tensor's allocation: the logical box, the padding of the physical box and of the planes"""
    import torch
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def _check_against_oracle(c, tag):
    """fields of the NumPy-mask path within n_max * 2^-52 of the oracle's on the same non-zero cells; the device-mask
    path (the padded layout of Grid3D) bit-equal to the NumPy-mask path; nothing off-mask or in the padding"""
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    want = _oracle(c)
    n_max = int(want.contribution_counts().max()) if want.contribution_counts().size else 0
    w_area = want.projected_area_fields()
    host, off = _device(c, c.mask), ~c.mask
    d_mask = hip.Grid3D(*c.mask.shape, c.dx, c.mask).d_mask
    dev = _device(c, d_mask)
    worst = 0.0

    area, d_area = host.projected_area_fields(), dev.projected_area_fields()
    for f in FACES:
        worst = max(worst, _compare('%s area %s' % (tag, f), area[f], w_area[f], n_max))
        assert not area[f][off].any(), f
        assert np.array_equal(d_area[f].cpu().numpy(), area[f], equal_nan=True), f
        assert int((_whole_storage(d_area[f]) != 0).sum()) == int(np.count_nonzero(area[f])), f     # padding untouched
    for fallback in (True, False):
        w_robin, w_scale = want.build_corrected_fields(c.base_h, fallback_to_base=fallback)
        robin, scale = host.build_corrected_fields(c.base_h, fallback_to_base=fallback)
        d_robin, d_scale = dev.build_corrected_fields(c.base_h, fallback_to_base=fallback)
        assert list(robin) == list(c.base_h) and list(d_robin) == list(c.base_h)
        for f in c.base_h:
            worst = max(worst, _compare('%s robin %s' % (tag, f), robin[f], w_robin[f], n_max),
                        _compare('%s scale %s' % (tag, f), scale[f], w_scale[f], n_max))
            assert not robin[f][off].any() and not scale[f][off].any(), f
            for d, h in ((d_robin[f], robin[f]), (d_scale[f], scale[f])):
                assert np.array_equal(d.cpu().numpy(), h, equal_nan=True), f
                assert int((_whole_storage(d) != 0).sum()) == int(np.count_nonzero(h)), f
            if c.base_h[f] == 0.0:
                assert not robin[f].any() and not scale[f].any(), f
    return worst, n_max, int(want.slots().offset[-1])


@pytest.mark.parametrize('seed', range(sm.FUZZ_SEEDS))
def test_fuzz_against_the_oracle(seed):
    """stlcorr_meshes.fuzz_case: boxes and plates on voxel planes, lattice-snapped soups, tilted and axis-aligned tubes;
    extents from 1 to 100 and ragged ones the layout pads; all-true, solid, holed and thin-walled masks; max_subdiv up to
    64.  test_oracle_stlcorr_golden.py::test_the_fuzz_stays_on_the_hard_cases asserts on the CPU how many of these cases
    have centroids exactly on voxel boundaries and how many are cut 16 deep or more."""
    c = sm.fuzz_case(seed)
    worst, n_max, nsub = _check_against_oracle(c, 'seed %d' % seed)
    print('STLCORR fuzz %2d: %s mesh, %s mask %s, max_subdiv %d, %d sub-triangles, n_max %d, largest relative difference '
          '%.3e (bound %.3e)' % (seed, c.mesh_kind, c.mask_kind, c.mask.shape, c.max_subdiv, nsub, n_max, worst, n_max * EPS))


def test_special_values_against_the_oracle():
    """the special_values mesh of the fixtures (NaN vertex, NaN and infinite area, area at area_epsilon, +-1e300 m, zero
    normal, a product that underflows to zero) on a holed mask and a negative origin, and a mesh whose bounding box is
    infinite (n clamps to max_subdiv; the reference raises there, the oracle states the device's rule).  Ordinary inputs
    with defined results: a cell is NaN only where the oracle's is, nothing lands off-mask."""
    import types
    g, base_h = _load('special_values')
    mask = g['mask'].copy()
    mask[2:4, 2:5, 2:4] = np.random.default_rng(5).random((2, 3, 2)) < 0.5
    tri = g['triangles'] - 2e-3
    inf = np.array([[[np.inf, 1e-3, 1e-3], [2e-3, 3e-3, 1e-3], [1e-3, 2e-3, 4e-3]],
                    [[1e-3, 1e-3, 1e-3], [2e-3, -np.inf, 1e-3], [1e-3, 2e-3, 4e-3]]])
    for name, mesh in (('fixture mesh', sm.mesh_of(tri, normals=g['normals'], areas=g['areas'])),
                       ('infinite span', sm.mesh_of(np.concatenate([tri[:1], inf, tri[8:]]),
                                                    normals=[[0.36, -0.48, 0.8]] * 4, areas=[2.1e-6, 1e-6, 1e-6, 4e-8]))):
        c = types.SimpleNamespace(mesh=mesh, mask=mask, origin=np.array([-2e-3, -2e-3, -2e-3]), dx=float(g['dx']),
                                  max_subdiv=int(g['max_subdiv']), area_epsilon=float(g['area_epsilon']), base_h=base_h)
        worst, n_max, nsub = _check_against_oracle(c, name)
        print('STLCORR special values, %s: %d sub-triangles, largest relative difference %.3e' % (name, nsub, worst))


def _abi_bin(tri, area, shape, origin, dx, max_subdiv, area_epsilon):
    """adi_stlcorr_count -> scan -> adi_stlcorr_bin on an all-true dense mask, straight on the C ABI;
    -> (offset, key, sub_area, slot_tri) as NumPy arrays"""
    import ctypes
    import torch
    from adi_thermal_fields_amd._lib import check, lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    d_tri = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.float64)).cuda()
    d_area = torch.from_numpy(np.ascontiguousarray(area, dtype=np.float64)).cuda()
    ntri = len(area)
    offset = torch.zeros(ntri + 1, dtype=torch.int64, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.adi_stlcorr_count(p(d_tri), p(d_area), ntri, dx, max_subdiv, area_epsilon,
                                ctypes.c_void_p(offset.data_ptr() + 8), stream))
    offset.cumsum_(0)
    nslot = int(offset[-1].item())
    nx, ny, nz = shape
    mask = torch.ones(nx * ny * nz, dtype=torch.uint8, device='cuda')
    key = torch.full((nslot,), -7, dtype=torch.int64, device='cuda')
    sub_area = torch.full((nslot,), -7.0, dtype=torch.float64, device='cuda')
    slot_tri = torch.full((nslot,), -7, dtype=torch.int64, device='cuda')
    check(lib.adi_stlcorr_bin(p(d_tri), p(d_area), p(offset), ntri, nslot, p(mask), nx, ny, nz, ny * nz, nz,
                              (ctypes.c_double * 3)(*[float(v) for v in origin]), dx, max_subdiv, p(key), p(sub_area),
                              p(slot_tri), stream))
    torch.cuda.synchronize()
    return offset.cpu().numpy(), key.cpu().numpy(), sub_area.cpu().numpy(), slot_tri.cpu().numpy()


# a sliver 4099 voxels long inside a 4100 x 2 x 2 grid: cut as deep as max_subdiv allows, every centroid in the grid
_SLIVER = np.array([[0.5, 0.3, 0.3], [4099.5, 0.6, 0.4], [2000.2, 1.7, 1.6]])
_SLIVER_GRID = (4100, 2, 2)


def _decode_case(tri, area, max_subdiv, area_epsilon=1e-16):
    import types
    from oracle import stlcorr_oracle as orc
    dx = 2.0 ** -10
    tri = np.asarray(tri, dtype=np.float64) * dx
    mesh = types.SimpleNamespace(triangles=tri, face_normals=np.zeros((len(tri), 3)), area_faces=np.asarray(area, float))
    want = orc.STLBoundaryCorrector(mesh, np.ones(_SLIVER_GRID, bool), (0.0, 0.0, 0.0), dx, max_subdiv=max_subdiv,
                                    area_epsilon=area_epsilon).slots(keep_centroids=False)
    offset, key, sub_area, slot_tri = _abi_bin(tri, area, _SLIVER_GRID, (0.0, 0.0, 0.0), dx, max_subdiv, area_epsilon)
    assert np.array_equal(offset, want.offset)
    assert np.all(want.cell >= 0)                                  # every centroid lands: every slot has a real key
    assert np.array_equal(slot_tri, want.tri)
    assert np.array_equal(sub_area, want.sub_area)
    wrong = np.nonzero(key != want.cell)[0]
    assert len(wrong) == 0, 'max_subdiv %d: %d of %d keys differ, the first at slot %d (device %d, oracle %d)' % (
        max_subdiv, len(wrong), len(key), wrong[0], key[wrong[0]], want.cell[wrong[0]])
    return len(key)


@pytest.mark.parametrize('max_subdiv', [2, 3, 7, 31, 64, 1000, 4096])
def test_slot_decode_at_depth(max_subdiv):
    """k_stl_bin's closed-form decode of (i, j, lower / upper) from the slot number, for EVERY slot of one triangle cut
    max_subdiv x max_subdiv, against the oracle's table written down by the loops (no square root)"""
    n = _decode_case([_SLIVER], [3.7e-3], max_subdiv)
    assert n == max_subdiv * max_subdiv


def test_slot_decode_steps_over_triangles_without_slots():
    """the binary search over repeated offsets: triangles at or below area_epsilon first, last, between two others and two
    in a row"""
    shifted = _SLIVER + [0.0, 0.05, -0.1]
    tri = [_SLIVER, _SLIVER, shifted, _SLIVER, _SLIVER, _SLIVER, shifted[[1, 2, 0]], _SLIVER]
    area = [0.0, 3.7e-3, 2.9e-3, 1e-9, 1e-9, 5.1e-3, 4.4e-3, 1e-9]
    assert _decode_case(tri, area, 7, area_epsilon=1e-9) == 4 * 49
    assert _decode_case(tri[:1] + tri[5:], area[:1] + area[5:], 33, area_epsilon=1e-9) == 2 * 33 * 33
